// rg_ppo_dev.inc -- the device code of rg_ppo.h's policy loss, once, for the feed-forward update (rg_ppo.hip) and for the
// recurrent one, which runs the same loss over a GRU's means: the Gaussian head of a sample in float64, a robot's KL, the
// finish of the loss and of the logstd gradient, and the penalty rule.  The GPU tests and the models under tests/ hold both
// updates to one definition of these (ppo_update_model.policy_head, move_penalty), so a clip term or another KL cut-off is
// written here and nowhere else.  Included after rg_agent_dev.inc, whose sums it calls, and so after the including file's
// `#pragma clang fp contract(off)`; rg_policy.h has been included.  Device functions and plain structs only, no kernel: each
// including file keeps its own named kernels around these bodies.

namespace {

constexpr int kHeadAct = RG_POLICY_MAX_ACT;   // the head's arrays
constexpr int kHeadPart = 1 + kHeadAct;       // a partial of the head: the loss sum, then the logstd gradient

struct LossCfg {
  int T, B, parts, act_dim, logstd_off, policy;   // parts: how many partials of kHeadPart; policy: 0 for the value loss
  double thr, coef;
};

struct AdamCfg {               // of an Adam kernel that takes no clip: adam_bias and adam_element (rg_agent_dev.inc) read it
  int count, pad0;
  double lr, b1, b2, eps;
};

// Sample n of the policy loss.  kBackward false: kls[n]; true: delta_mean[n], and the sample's terms of the loss and of the
// logstd gradient are added to loss and gls.  inv = 1 / (T B).  A sample that is not live (the padding of a tile) reads
// nothing of the rollout and still gets a zero delta.  S is the caller's view of the sample:
//   cfg()   the descriptor with act_dim, B, logstd_off, c, thr and coef, read where they are used, as the callers' own text did
//   mask(n), logstd0(k), mean(n, k), mean0(n, k), action(n, k), adv(n), scal(), robot_kl(b), penalty()   the loads
//   keep_kl(n, v), keep_delta(n, k, v)                                                                  the stores
template <bool kBackward, typename S>
__device__ __forceinline__ void gaussian_head(const S &s, const float *__restrict__ P, const int n, const bool live, const double inv, double &loss,
                                              double (&gls)[kHeadAct]) {
  const int act_dim = s.cfg().act_dim;
  const bool valid = live && s.mask(n) != 0;
  double kl = 0.0, lp = 0.0, lp0 = 0.0;
  double z[kHeadAct], D[kHeadAct], q[kHeadAct], sg[kHeadAct], mu[kHeadAct];
#pragma unroll
  for (int k = 0; k < kHeadAct; k++) {
    z[k] = D[k] = q[k] = mu[k] = 0.0;
    sg[k] = 1.0;
    if (k < act_dim && live) {
      const double ls = (double)P[s.cfg().logstd_off + k], ls0 = (double)s.logstd0(k);
      const double s1 = exp(ls), s0 = exp(ls0);
      const double m1 = (double)s.mean(n, k), m0 = (double)s.mean0(n, k);
      const double dk = m1 - m0;
      const double qk = (s0 * s0 + dk * dk) / (s1 * s1);
      kl = kl + ((qk - 1.0) + 2.0 * (ls - ls0));
      if (kBackward) {
        const double a = (double)s.action(n, k);
        const double zk = (a - m1) / s1, z0 = (a - m0) / s0;
        lp = lp + (-s.cfg().c * ls - 0.5 * (zk * zk));
        lp0 = lp0 + (-s.cfg().c * ls0 - 0.5 * (z0 * z0));
        z[k] = zk;
      }
      D[k] = dk; q[k] = qk; sg[k] = s1; mu[k] = m1;
    }
  }
  kl = 0.5 * kl;
  if (!kBackward) {
    if (live) s.keep_kl(n, valid ? kl : 0.0);
  } else {
    double ratio = 0.0, advn = 0.0, gb = 0.0;
    if (valid) {
      ratio = exp(lp - lp0);
      advn = ((double)s.adv(n) - s.scal()[1]) / s.scal()[2];
      const double klb = s.robot_kl(n % s.cfg().B);
      gb = s.penalty() + (klb > s.cfg().thr ? 2.0 * s.cfg().coef * (klb - s.cfg().thr) : 0.0);
      loss = loss + ratio * advn;
    }
#pragma unroll
    for (int k = 0; k < kHeadAct; k++) {
      if (k < act_dim) {
        float dlt = 0.0f;
        if (valid) {
          const double dmu = (-advn * ratio * z[k] / sg[k] + gb * D[k] / (sg[k] * sg[k])) * inv;
          dlt = (float)(dmu * (1.0 - mu[k] * mu[k]));
          gls[k] = gls[k] + (-advn * ratio * (z[k] * z[k] - s.cfg().c) + gb * (1.0 - q[k])) * inv;
        }
        s.keep_delta(n, k, dlt);
      }
    }
  }
}

// KL_b = (sum_t kls[t][b]) / T, t in order
__device__ __forceinline__ void robot_kl_element(const int T, const int B, const double *__restrict__ kls, double *__restrict__ out, const int b) {
  if (b >= B) return;
  double s = 0.0;
  for (int t = 0; t < T; t++) s = s + kls[(size_t)t * B + b];
  out[b] = s / (double)T;
}

// the loss from the float64 partials, every thread of the workgroup in it: the mean over the T B samples; for the policy, minus
// that, plus the penalty terms' mean over the robots, and the logstd gradient into grad
__device__ __forceinline__ void loss_finish(const LossCfg &c, const int parts, const bool policy, const double *__restrict__ part,
                                            const double *__restrict__ klr, const double *__restrict__ penalty, float *__restrict__ grad,
                                            double *__restrict__ loss_out, double *__restrict__ loss_out2, double *sh) {
  const double s1 = strided_sum(part, parts, kHeadPart, sh);
  const double inv = 1.0 / ((double)c.T * (double)c.B);
  double loss = s1 * inv;
  if (policy) {
    const double pen = *penalty;
    double s2 = 0.0;
    for (int b = threadIdx.x; b < c.B; b += kAgentThreads) {
      const double k = klr[b], over = k - c.thr;
      s2 = s2 + (pen * k + (k > c.thr ? c.coef * (over * over) : 0.0));
    }
    s2 = block_sum(s2, sh);
    loss = -(s1 * inv) + s2 / (double)c.B;
#pragma unroll
    for (int k = 0; k < kHeadAct; k++) {
      if (k < c.act_dim) {   // uniform
        const double gk = strided_sum(part + 1 + k, parts, kHeadPart, sh);
        if (threadIdx.x == 0) grad[c.logstd_off + k] = (float)gk;
      }
    }
  }
  if (threadIdx.x == 0) {
    *loss_out = loss;
    if (loss_out2) *loss_out2 = loss;
  }
}

// the penalty after an update: the KL's mean over the robots and the penalty it leaves (x 1.5 above 1.3 target, / 1.5 below 0.7)
struct PenaltyMove { double change, penalty; };

__device__ __forceinline__ PenaltyMove move_penalty(const double kl_sum, const int B, const double target, const double *penalty) {
  const double change = kl_sum / (double)B;
  double pen = *penalty;
  if (change > 1.3 * target) pen = pen * 1.5;
  else if (change < 0.7 * target) pen = pen / 1.5;
  return PenaltyMove{change, pen};
}

}  // namespace
