"""Evidence of the carried record pipeline (Record pipeline carried across the tables):
the N = 20 kernels' resources, and the disassembly of the headline kernel's ADMM loop from its
header through both solve-step loops with the two ways between the solves.

    python tools/isa_record_pipe.py resources [lib.so]   # registers, scratch, spills, non-check path
    python tools/isa_record_pipe.py loops [lib.so]       # the excerpt (profiles/r07/record_pipe/)
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from test_isa_hot_loops import _shortest, disassemble, shortest_iteration  # noqa: E402
from test_isa_record_pipeline import HEADLINE, _exits, _loads, _solve_loops  # noqa: E402
from test_kernel_resources import LIB, kernel_resources  # noqa: E402

N20 = "qp_batch_kernelILi2ELi4ELb"


def resources(lib):
    print("# python tools/isa_record_pipe.py resources: the one-wave (2, 4) KM_LDS kernels of libmpcqp.so")
    print("# (...ELi0ELi0E: restart per solve, ...ELi0ELi1E: carried pipeline); AMDHSA metadata, then the")
    print("# shortest non-check iteration of tests/test_isa_hot_loops.py (its loop bodies counted once)")
    for name, v in sorted(kernel_resources(lib).items()):
        if N20 in name and "ELi0ELi" in name:
            print(name, "vgpr_count", v["vgpr_count"], "agpr_count", v["agpr_count"], "scratch_bytes",
                  v["private_segment_fixed_size"], "vgpr_spill_count", v["vgpr_spill_count"],
                  "sgpr_spill_count", v["sgpr_spill_count"])
    for name, ins in sorted(disassemble(lib).items()):
        if N20 in name and "ELi0ELi" in name:
            path = shortest_iteration(ins)
            print(name, "non-check iteration: instructions", len(path), "v_readlane",
                  sum(t.startswith("v_readlane") for t in path), "s_load",
                  sum(t.startswith("s_load") for t in path))


def loops(lib):
    (name, ins), = [(n, i) for n, i in disassemble(lib).items() if HEADLINE.search(n)]
    idx, (h, e), fwd, bwd = _solve_loops(ins)
    tgt = {a: i for a, i in idx.items()}
    print("# python tools/isa_record_pipe.py loops:", name)
    print("# ADMM loop [%d, %d], forward step loop [%d, %d], backward step loop [%d, %d] (instruction"
          % (h, e, fwd[0], fwd[1], bwd[0], bwd[1]))
    print("# indices); buffer loads from the forward loop's exit to the backward loop's header: %d; from the"
          % _loads(ins, idx, _exits(ins, idx, *fwd), bwd[0], h, e))
    print("# backward loop's exit over the back edge to the forward loop's header, check blocks skipped: %d"
          % _loads(ins, idx, _exits(ins, idx, *bwd), fwd[0], h, e))

    def show(i):
        _, t, b = ins[i]
        mark = {h: "ADMM header", fwd[0]: "forward loop header", fwd[1]: "forward loop back edge",
                bwd[0]: "backward loop header", bwd[1]: "backward loop back edge", e: "ADMM back edge"}.get(i)
        print("%6d  %s%s%s" % (i, t, "   -> %d" % tgt[b] if b in tgt else "", "    ; <== " + mark if mark else ""))

    print("\n## 1. ADMM loop header through the end of the backward step loop (every instruction)")
    for i in range(h, bwd[1] + 1):
        show(i)
    print("\n## 2. backward loop exit -> ADMM back edge -> forward loop header, shortest way (skips the")
    print("##    check blocks): branches, waits, record loads and spill reloads only")
    for a in _exits(ins, idx, *bwd):
        for i in _shortest(ins, idx, a, fwd[0], h, e):
            if ins[i][1].startswith(("s_cbranch", "s_branch", "s_waitcnt", "buffer_load", "v_readlane", "s_load")):
                show(i)


if __name__ == "__main__":
    {"resources": resources, "loops": loops}[sys.argv[1]](sys.argv[2] if len(sys.argv) > 2 else LIB)
