// rg_goto_dev.inc -- device code of the go-to-target task shared by rg_goto.hip (the tick) and rg_episode.hip (the
// observation of a reset on the device): the kernel-side configuration, the path view, and steps 1 and 2 of the tick of
// include/rg_goto.h -- window, visible points, chain, interpolation -- for one robot on one 64-lane wave; and the host-side
// checks and fills of rg_goto_config (on the helpers of rg_host.h).  Included after `#pragma clang fp contract(off)`, inside the including file's anonymous namespace.

constexpr int kWave = 64;
constexpr int kMaxVis = RG_GOTO_MAX_VISIBLE;

struct GotoCfg {
  int B, n_max, ncp, ncheck, max_visible;
  double wh, wt, wb, wd;
  double max_err, inv_max_err, prog_window, prog_limit, radius, penalty, cp_reward, max_steps, brk;
  double lo[2], hi[2];
  float off[3];
};

struct Paths {
  const double *x, *y, *s;
  const int *fsx;
  const double *hdr;
};

inline bool paths_ok(const rg_goto_path_ptrs *p) { return p && p->x && p->y && p->s && p->first_same_x && p->hdr; }

inline Paths to_paths(const rg_goto_path_ptrs *p) { return {p->x, p->y, p->s, p->first_same_x, p->hdr}; }

// (d, i) <- the lexicographic minimum over the wave, in every lane
__device__ __forceinline__ void wave_argmin(double &d, int &i) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {
    const double od = __shfl_xor(d, m);
    const int oi = __shfl_xor(i, m);
    if (od < d || (od == d && oi < i)) { d = od; i = oi; }
  }
}

// yaw of the quaternion (x, y, z, w): atan2(R[1][0], R[0][0])
__device__ __forceinline__ double yaw_of_quat(double x, double y, double z, double w) {
  return atan2(2 * (x * y + z * w), 1 - 2 * (y * y + z * z));
}

__device__ __forceinline__ double yaw_of(const double *__restrict__ sim, size_t sB, int b) {
  return yaw_of_quat(sim[(RG_SRB_ROW_QUAT + 0) * sB + b], sim[(RG_SRB_ROW_QUAT + 1) * sB + b], sim[(RG_SRB_ROW_QUAT + 2) * sB + b],
                     sim[(RG_SRB_ROW_QUAT + 3) * sB + b]);
}

// Steps 1 (the stores) and 2 of the tick for robot b with n path points X, Y: the robot at (px, py, yaw), its last pose
// (ox, oy, oyaw).  Writes obs and the observation rows of the task state; leaves the nearest path point to the new pose
// (bd, bi) and to the last one (bpi) and the count of points in the window.  vx .. cs: kMaxVis doubles of LDS each.  The
// whole wave calls it (it holds __syncthreads and cross-lane operations).
__device__ __forceinline__ void goto_observe(const GotoCfg &c, const int b, const int lane, const int n, double *__restrict__ task,
                                             const double *X, const double *Y, const double px, const double py, const double yaw,
                                             const double ox, const double oy, const double oyaw, float *__restrict__ obs, double *vx,
                                             double *vy, double *cx, double *cy, double *cs, double &bd, int &bi, int &bpi) {
  const size_t sB = (size_t)c.B;
  const double inf = __builtin_inf();
  double sn, cz;
  sincos(yaw, &sn, &cz);
  // the window's corners in the world, clockwise
  const double lcx[4] = {c.wd + c.wh, c.wd + c.wh, c.wd, c.wd};
  const double lcy[4] = {c.wt / 2, -(c.wt / 2), -(c.wb / 2), c.wb / 2};
  double wx[4], wy[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    wx[e] = px + (cz * lcx[e] - sn * lcy[e]);
    wy[e] = py + (sn * lcx[e] + cz * lcy[e]);
  }
  // 2a. one pass over the path: nearest point to pos and to prev_pos, and the visible points
  double bpd = inf;
  bd = inf;
  bi = INT_MAX; bpi = INT_MAX;
  int count = 0;
  for (int base = 0; base < n; base += kWave) {
    const int i = base + lane;
    const bool valid = i < n;
    const double x = valid ? X[i] : 0.0, y = valid ? Y[i] : 0.0;
    const double dx = x - px, dy = y - py, dn = sqrt(dx * dx + dy * dy);
    const double ex = x - ox, ey = y - oy, en = sqrt(ex * ex + ey * ey);
    if (valid && dn < bd) { bd = dn; bi = i; }
    if (valid && en < bpd) { bpd = en; bpi = i; }
    bool vis = valid;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int f = (e + 1) & 3;
      const double cr = (wx[f] - wx[e]) * (y - wy[e]) - (wy[f] - wy[e]) * (x - wx[e]);
      vis = vis && cr <= 0.0;
    }
    const unsigned long long m = __ballot(vis);
    const int rank = count + __popcll(m & ((1ull << lane) - 1ull));
    if (vis && rank < c.max_visible) {   // rank < max_visible <= kMaxVis: never past the arrays
      vx[rank] = cz * dx + sn * dy;
      vy[rank] = cz * dy - sn * dx;
    }
    count += __popcll(m);
  }
  wave_argmin(bd, bi);
  wave_argmin(bpd, bpi);
  const int nvis = count < c.max_visible ? count : c.max_visible;
  __syncthreads();
  // 2b. sort_points
  const bool has0 = lane < nvis, has1 = lane + kWave < nvis;
  const double p0x = has0 ? vx[lane] : 0.0, p0y = has0 ? vy[lane] : 0.0;
  const double p1x = has1 ? vx[lane + kWave] : 0.0, p1y = has1 ? vy[lane + kWave] : 0.0;
  bool free0 = has0, free1 = has1;
  int clen = 0;
  double acc = 0.0;
  if (nvis > 0) {
    double tx = 0.0, ty = 0.0;   // the chain's tail; the origin before the first point
    for (;;) {
      const double a0 = p0x - tx, b0 = p0y - ty, a1 = p1x - tx, b1 = p1y - ty;
      double d = free0 ? sqrt(a0 * a0 + b0 * b0) : inf;
      int w = lane;
      const double d1 = free1 ? sqrt(a1 * a1 + b1 * b1) : inf;
      if (d1 < d) { d = d1; w = lane + kWave; }
      wave_argmin(d, w);
      if (clen > 0) {
        if (d > c.brk) break;
        acc = acc + d;
      }
      const int owner = w & (kWave - 1), slot = w >> 6;
      tx = __shfl(slot ? p1x : p0x, owner);
      ty = __shfl(slot ? p1y : p0y, owner);
      if (lane == owner) { if (slot) free1 = false; else free0 = false; }
      if (lane == 0) { cx[clen] = tx; cy[clen] = ty; cs[clen] = acc; }
      clen++;
      if (clen == nvis) break;
    }
  }
  __syncthreads();
  // 2c. interpolate_points, one output point per lane
  const bool fresh = clen >= 2 && acc > 0.0;
  if (lane < c.ncp) {
    double qx = task[(RG_GOTO_ROW_OBS + 2 * lane) * sB + b], qy = task[(RG_GOTO_ROW_OBS + 2 * lane + 1) * sB + b];
    if (fresh) {
      const double seg = c.ncp > 1 ? acc / (double)(c.ncp - 1) : 0.0;
      const double t = (double)lane * seg;
      if (!(t > acc + 1e-6)) {
        if (t >= acc) { qx = cx[clen - 1]; qy = cy[clen - 1]; }
        else {
          int k = 0;
          while (k < clen - 2 && !(t < cs[k + 1])) k++;
          const double fr = (t - cs[k]) / (cs[k + 1] - cs[k]);
          qx = cx[k] + fr * (cx[k + 1] - cx[k]);
          qy = cy[k] + fr * (cy[k + 1] - cy[k]);
        }
        task[(RG_GOTO_ROW_OBS + 2 * lane) * sB + b] = qx;
        task[(RG_GOTO_ROW_OBS + 2 * lane + 1) * sB + b] = qy;
      }
    }
    obs[(2 * lane) * sB + b] = (float)qx;
    obs[(2 * lane + 1) * sB + b] = (float)qy;
  }
  if (lane == 0) {
    task[(RG_GOTO_ROW_PREV + 0) * sB + b] = ox; task[(RG_GOTO_ROW_PREV + 1) * sB + b] = oy; task[(RG_GOTO_ROW_PREV + 2) * sB + b] = oyaw;
    task[(RG_GOTO_ROW_POS + 0) * sB + b] = px; task[(RG_GOTO_ROW_POS + 1) * sB + b] = py; task[(RG_GOTO_ROW_POS + 2) * sB + b] = yaw;
    if (count > c.max_visible) task[RG_GOTO_ROW_OVERFLOW * sB + b] = 1.0;
    task[RG_GOTO_ROW_VISIBLE * sB + b] = (double)count;
    task[RG_GOTO_ROW_CHAIN * sB + b] = (double)clen;
    task[RG_GOTO_ROW_LATCHED * sB + b] = fresh ? 1.0 : 0.0;
  }
}

// GotoCfg of a validated rg_goto_config (host)
inline void goto_fill_cfg(const rg_goto_config *cfg, int batch, GotoCfg &c) {
  c.B = batch; c.n_max = cfg->n_max; c.ncp = cfg->num_cam_pts; c.ncheck = cfg->num_checkpoints; c.max_visible = cfg->max_visible;
  c.wh = cfg->window_height; c.wt = cfg->window_top_width; c.wb = cfg->window_bottom_width; c.wd = cfg->window_distance;
  c.max_err = cfg->max_track_err; c.inv_max_err = 1.0 / cfg->max_track_err;
  c.prog_window = cfg->progress_window; c.prog_limit = cfg->progress_limit; c.radius = cfg->target_radius;
  c.penalty = cfg->time_penalty; c.cp_reward = cfg->checkpoint_reward_total / (double)cfg->num_checkpoints;
  c.max_steps = cfg->max_time / (cfg->dt_sim * (double)cfg->substeps);
  c.brk = cfg->continuity_break;
  for (int i = 0; i < 2; i++) { c.lo[i] = cfg->action_low[i]; c.hi[i] = cfg->action_high[i]; }
  for (int i = 0; i < 3; i++) c.off[i] = (float)cfg->cmd_offset[i];
}

// The checks of rg_goto_create on the configuration and the batch; false: err names the field (host)
inline bool goto_validate(const rg_goto_config *cfg, int32_t batch, std::string &err) {
  const RealField reals[] = {{"window_height", &cfg->window_height, 1, kPositive}, {"window_top_width", &cfg->window_top_width, 1, kPositive},
                             {"window_bottom_width", &cfg->window_bottom_width, 1, kPositive}, {"window_distance", &cfg->window_distance, 1, kFinite},
                             {"max_track_err", &cfg->max_track_err, 1, kPositive}, {"progress_window", &cfg->progress_window, 1, kPositive},
                             {"progress_limit", &cfg->progress_limit, 1, kPositive}, {"target_radius", &cfg->target_radius, 1, kPositive},
                             {"time_penalty", &cfg->time_penalty, 1, kFinite}, {"checkpoint_reward_total", &cfg->checkpoint_reward_total, 1, kFinite},
                             {"max_time", &cfg->max_time, 1, kPositive}, {"continuity_break", &cfg->continuity_break, 1, kPositive},
                             {"action_low", cfg->action_low, 2, kFinite}, {"action_high", cfg->action_high, 2, kFinite},
                             {"cmd_offset", cfg->cmd_offset, 3, kFinite}, {"dt_sim", &cfg->dt_sim, 1, kPositive}};
  if (!check_abi("config.", cfg->abi_version, RG_GOTO_ABI_VERSION, err) || !check_reserved("config.", "reserved0", cfg->reserved0, err) ||
      !check_reserved("config.", "reserved1", cfg->reserved1, err) || !check_batch(batch, RG_GOTO_MAX_BATCH, err) ||
      !check_reals("config.", reals, err))
    return false;
  for (int i = 0; i < 2; i++)
    if (cfg->action_low[i] > cfg->action_high[i]) {
      char msg[200];
      snprintf(msg, sizeof(msg), "config.action_low[%d]: %g above action_high[%d] = %g", i, cfg->action_low[i], i, cfg->action_high[i]);
      err = msg;
      return false;
    }
  const IntField ints[] = {{"substeps", cfg->substeps, 1, RG_SRB_MAX_SUBSTEPS}, {"num_cam_pts", cfg->num_cam_pts, 1, RG_GOTO_MAX_CAM_PTS},
                           {"num_checkpoints", cfg->num_checkpoints, 1, RG_GOTO_MAX_CHECKPOINTS}, {"n_max", cfg->n_max, 2, RG_GOTO_MAX_PATH},
                           {"max_visible", cfg->max_visible, 2, RG_GOTO_MAX_VISIBLE}};
  return check_ints("config.", ints, err);
}
