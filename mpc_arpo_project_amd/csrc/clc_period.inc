// clc_period.inc -- the period kernel of the continuous-time closed loop, included by
// closed_loop.hip once per instantiation (see there for what a period is):
//   CLC_PERIOD_KERNEL  the kernel's name
//   CLC_PERIOD_TRACK   0 / 1: the compile-time flag of the run summary (TRACK below); the tracked
//                      kernel takes the summary's buffers and tolerances as one more argument
// A textual instantiation, not a template body inside two wrappers: behind a wrapper the
// untracked kernel came out with its instructions scheduled differently, and mpcqp_clc_period
// without tracking is to run the code it ran before the summary existed.
__global__ void __launch_bounds__(64) CLC_PERIOD_KERNEL(
    ClDev d, PlantConsts pc, int isDeltaV, const int32_t* status, const double* x_sol, int n,
    int u0, double* x_true, double* ctrl_prev, double* xintf, double* xest, int32_t* done,
    int32_t* iterm, int32_t* ctrl_seq, double* ctrl_out, const double* noise, double* z_out,
    double* u_applied, double t_start, double dt, int i_start, int nsub, double* traj
#if CLC_PERIOD_TRACK
    , TrackC tc) {
#else
    ) {
  const TrackC tc{};  // named by the discarded branches only
#endif
  constexpr bool TRACK = CLC_PERIOD_TRACK;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= d.B) return;
  const mpcqp_cl_scenario& s = d.sc;
  if (done[b]) {
    ctrl_seq[b] = 0;
    return;
  }
  const double* xe = xest + (size_t)b * 6;
  double c0, c1, xi = xintf[b];
  const int seq = select_control(s, status[b], x_sol + (size_t)b * n + u0, xe, xi, c0, c1);
  xintf[b] = xi;
  ctrl_seq[b] = seq;
  ctrl_out[(size_t)b * 2] = c0;
  ctrl_out[(size_t)b * 2 + 1] = c1;
  double* up = ctrl_prev + (size_t)b * NU;
  const double p0 = up[0], p1 = up[1];
  if (u_applied) {
    u_applied[(size_t)b * 2] = p0;
    u_applied[(size_t)b * 2 + 1] = p1;
  }
  double w[NX] = {0, 0, 0, 0};
  if (noise)
    for (int i = 0; i < NX; ++i) w[i] = noise[(size_t)b * NX + i];
  double x[NX];
  for (int i = 0; i < NX; ++i) x[i] = x_true[(size_t)b * NX + i];
  double t = t_start;
  int stop = -1;
  int32_t succ = 0, i_end = 0;
  double ferr = 0.0;
  // the summary in registers: track_state writes through a one-chaser view of these two
  const Track lt{nullptr, &succ, nullptr, &ferr, tc.dist_tol, tc.ang_tol, tc.rad2deg, 1};
  if constexpr (TRACK) {
    succ = tc.success[b];
    ferr = tc.final_err[b];
    i_end = iterm[b];
  }
  for (int k = 0; k < nsub; ++k) {
    if (k > 0 && terminated(s, x)) {
      stop = i_start + k;
      break;
    }
    if constexpr (TRACK)
      track_state(s, x, lt, 0);
    const double t1 = add(t, dt);
    const double ua = isDeltaV ? 0.0 : (k == 0 ? p0 : c0);
    const double ub = isDeltaV ? 0.0 : (k == 0 ? p1 : c1);
    rk45_interval(pc, t, t1, x, ua, ub);
    if (isDeltaV && k == 0) {
      x[2] = add(x[2], p0);
      x[3] = add(x[3], p1);
    }
    for (int i = 0; i < NX; ++i) x[i] = add(x[i], w[i]);
    if (traj)
      for (int i = 0; i < NX; ++i) traj[((size_t)b * nsub + k) * NX + i] = x[i];
    if (k == 0) {
      double* xw = xest + (size_t)b * 6;
      for (int i = 0; i < NX; ++i) xw[i] = x[i];
      xw[4] = 0.0;
      xw[5] = 0.0;
      if (z_out) measure(x, z_out + (size_t)b * 2);
    }
    t = t1;
  }
  if (stop < 0 && terminated(s, x)) stop = i_start + nsub;
  if (stop >= 0) {
    done[b] = 1;
    iterm[b] = stop;
  }
  if constexpr (TRACK) {
    int32_t cnt = (stop >= 0 ? stop : i_start + nsub) - i_start;
    if (stop < 0) {
      track_state(s, x, lt, 0);
      if (i_start + nsub + 1 == i_end) ++cnt;
    }
    tc.success[b] = succ;
    tc.final_err[b] = ferr;
    if (seq != 1) tc.n_fallback[b] += 1;
    tc.n_ctrl[(size_t)b * 3 + (seq - 1)] += cnt;
  }
  for (int i = 0; i < NX; ++i) x_true[(size_t)b * NX + i] = x[i];
  up[0] = c0;
  up[1] = c1;
}
