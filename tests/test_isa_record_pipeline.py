"""Build-time ISA guard of the carried record pipeline (no GPU needed; engine.hip RP_CARRY).

The headline kernel -- the one-wave (2, 4) paired KM_LDS kernel with the carried pipeline, what an
N = 20 handle launches -- must load at most one record set (five buffer loads) between its solves,
not the three of a restart: on the way from the forward step loop into the backward one, and from
the backward loop through an iteration end that skips every check block into the next iteration's
forward loop.  (As built it loads none there: sets a and b are carried, and every rotation of a
step loop loads its own set c.)  A restart (15 loads) would mean the carry-over has been lost to a
code change.

The paths are shortest paths in the control-flow graph of the disassembled gfx950 code object, from
every exit of a step loop (a branch out of it, or the fall-through behind its back edge) to the
header of the next one; the exit with the most loads on its path counts.
"""
import re

import pytest

from test_isa_hot_loops import _shortest, _step_loops, _succ, disassemble, loops

# qp_batch_kernel<2, 4, true, KM_LDS, RP_CARRY>
HEADLINE = re.compile(r"qp_batch_kernelILi2ELi4ELb1ELi0ELi1E")


@pytest.fixture(scope="module")
def headline():
    k = {n: ins for n, ins in disassemble().items() if HEADLINE.search(n)}
    assert len(k) == 1, sorted(k)
    return next(iter(k.values()))


def _exits(ins, idx, h, e):
    """indices outside [h, e] that an instruction of the loop [h, e] continues at"""
    return sorted({j for i in range(h, e + 1) for j in _succ(ins, i, idx) if not h <= j <= e})


def _loads(ins, idx, starts, target, lo, hi):
    """buffer loads on the shortest path from each start to target inside [lo, hi]: the largest"""
    worst = 0
    for a in starts:
        path = _shortest(ins, idx, a, target, lo, hi)
        worst = max(worst, sum(ins[i][1].startswith("buffer_load") for i in path[:-1]))
    return worst


def _solve_loops(ins):
    idx = {a: i for i, (a, _, _) in enumerate(ins)}
    h, e = max(loops(ins), key=lambda x: x[1] - x[0])  # the ADMM iteration loop
    # a step loop may have more than one back edge: the loop of a header is its widest
    by_header = {}
    for sh, se in _step_loops(ins):
        if h < sh and se < e:
            by_header[sh] = max(se, by_header.get(sh, se))
    fwd, bwd = sorted(by_header.items())[:2]
    return idx, (h, e), fwd, bwd


def test_carried_kernels_within_budget_and_without_vector_spills():
    """the carried variants by name (test_kernel_resources looks at the first kernel that matches
    the (2, 4) KM_LDS prefix, whichever variant the metadata lists first)"""
    from test_kernel_resources import _header_budget, kernel_resources

    carried = {n: v for n, v in kernel_resources().items()
               if re.search(r"qp_batch_kernelILi2ELi4ELb[01]ELi0ELi1E", n)}
    assert len(carried) == 2, sorted(carried)  # paired and unpaired
    for n, v in carried.items():
        assert int(v["vgpr_spill_count"]) == 0, (n, v)
        assert int(v["vgpr_count"]) <= _header_budget("MPCQP_MAX_KERNEL_REGS"), (n, v)
        assert int(v["private_segment_fixed_size"]) <= _header_budget("MPCQP_MAX_KERNEL_SCRATCH"), (n, v)


def test_step_loops_load_three_sets_a_rotation(headline):
    """the two step loops are there and are rotations of three steps with a set's reload each"""
    _, _, fwd, bwd = _solve_loops(headline)
    for h, e in (fwd, bwd):
        body = [t for _, t, _ in headline[h:e + 1]]
        assert sum(t.startswith("buffer_load") for t in body) == 15, (h, e)
        assert sum(t.startswith("ds_add_f64") for t in body) == 9, (h, e)  # paired: 3 a step


def test_forward_to_backward_loads_at_most_one_set(headline):
    ins = headline
    idx, (h, e), fwd, bwd = _solve_loops(ins)
    assert _loads(ins, idx, _exits(ins, idx, *fwd), bwd[0], h, e) <= 5


def test_backward_to_next_forward_loads_at_most_one_set_on_a_non_check_iteration(headline):
    ins = headline
    idx, (h, e), fwd, bwd = _solve_loops(ins)
    # the forward loop lies in front of the backward one, so the way leads over the back edge of
    # the ADMM loop; the shortest way skips the check blocks
    assert fwd[0] < bwd[0]
    assert _loads(ins, idx, _exits(ins, idx, *bwd), fwd[0], h, e) <= 5
