// rg_host.h -- the host helpers that every translation unit of the library but the controller's shares: the device scope and
// the device preamble of a create, the workspace arithmetic, the layout rules, the checks of a configuration's fields (and
// of a whole rg_policy_config, rg_rnn_config or rg_ppo_config, where the header that declares it has been included first)
// and the error helpers.  Every message is formed here once; the callers give the prefix ("config.", "policy_cfg.",
// "rnn_cfg.", "" for an argument) and their API's status codes.
// rg_mpc.hip does not include it, so the source hash behind profiles/ does not move.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <optional>
#include <string>

namespace {

// The calling thread's current device is restored on scope exit (rg_mpc.h conventions).
struct DeviceScope {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DeviceScope(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) { err = hipSetDevice(dev); switched = err == hipSuccess && prev >= 0; }
  }
  ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
};

// The device preamble of a create: a device exists, `device` is one of them and, where the caller gives a scope to enter (its
// own, because it lives to the end of the create), the switch went through.  0, every API's OK, or the status of the caller's
// that applies, with the text in err.
inline int enter_device(int device, std::optional<DeviceScope> *scope, int st_no_device, int st_invalid, int st_hip, std::string &err) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { err = "no HIP device available"; return st_no_device; }
  if (device < 0 || device >= ndev) { err = "device index out of range"; return st_invalid; }
  if (!scope) return 0;
  scope->emplace(device);
  if ((*scope)->err != hipSuccess) { err = std::string("hipSetDevice failed: ") + hipGetErrorString((*scope)->err); return st_hip; }
  return 0;
}

inline size_t round8(size_t n) { return (n + 7) & ~(size_t)7; }

template <typename T>
T *ws_at(void *workspace, size_t off) { return reinterpret_cast<T *>(static_cast<char *>(workspace) + off); }

// the layout rule of rg_policy.h for one network: W[in][out] then b[out] per layer, the nh hidden layers then the head.
// Returns the floats the network takes; entries past layer nh are left as they are.
inline int layer_layout(int first, const int32_t *widths, int nh, int head, int32_t *in, int32_t *out, int32_t *w, int32_t *b) {
  int off = 0, prev = first;
  for (int l = 0; l <= nh; l++) {
    const int width = l < nh ? widths[l] : head;
    in[l] = prev; out[l] = width;
    w[l] = off; off += prev * width;
    b[l] = off; off += width;
    prev = width;
  }
  return off;
}

// ---- the checks of a configuration ----------------------------------------------------------------------------------------

inline bool check_abi(const char *prefix, int got, int want, std::string &err) {
  if (got == want) return true;
  char msg[200];
  snprintf(msg, sizeof(msg), "%sabi_version: %d, this library is version %d", prefix, got, want);
  err = msg;
  return false;
}

inline bool check_reserved(const char *prefix, const char *name, int value, std::string &err) {
  if (value == 0) return true;
  err = std::string(prefix) + name + ": must be 0";
  return false;
}

inline bool check_batch(int batch, int max, std::string &err) {
  if (batch >= 1 && batch <= max) return true;
  char msg[96];
  snprintf(msg, sizeof(msg), "batch: %d outside [1, %d]", batch, max);
  err = msg;
  return false;
}

struct IntField { const char *name; int v, lo, hi; };

template <size_t N>
bool check_ints(const char *prefix, const IntField (&fields)[N], std::string &err) {
  for (const IntField &f : fields)
    if (f.v < f.lo || f.v > f.hi) {
      char msg[200];
      snprintf(msg, sizeof(msg), "%s%s: %d outside [%d, %d]", prefix, f.name, f.v, f.lo, f.hi);
      err = msg;
      return false;
    }
  return true;
}

// the width list of one network: the n layers in use within [1, max_width], the entries past them 0
inline bool check_widths(const char *prefix, const char *name, const int32_t *w, int n, int max_layers, int max_width, std::string &err) {
  char msg[200];
  for (int k = 0; k < max_layers; k++) {
    if (k < n && (w[k] < 1 || w[k] > max_width)) {
      snprintf(msg, sizeof(msg), "%s%s[%d]: %d outside [1, %d]", prefix, name, k, w[k], max_width);
      err = msg;
      return false;
    }
    if (k >= n && w[k] != 0) {
      snprintf(msg, sizeof(msg), "%s%s[%d]: %d must be 0 past the %d layers in use", prefix, name, k, w[k], n);
      err = msg;
      return false;
    }
  }
  return true;
}

enum RealKind { kNonNegative, kBelowOne, kPositive, kUnit, kUnitPositive, kFinite };   // >= 0; [0, 1); > 0; [0, 1]; (0, 1]; any finite
struct RealField { const char *name; const double *p; int n; RealKind kind; };   // a scalar: &cfg->x, 1; an array (n > 1) is kFinite

template <size_t N>
bool check_reals(const char *prefix, const RealField (&fields)[N], std::string &err) {
  const char *want[] = {">= 0", "in [0, 1)", "> 0", "in [0, 1]", "in (0, 1]", "finite"};
  for (const RealField &f : fields)
    for (int i = 0; i < f.n; i++) {
      const double v = f.p[i];
      bool ok = std::isfinite(v);
      if (ok && f.kind != kFinite) ok = v >= 0;
      if (ok && f.kind == kBelowOne) ok = v < 1;
      if (ok && (f.kind == kPositive || f.kind == kUnitPositive)) ok = v > 0;
      if (ok && (f.kind == kUnit || f.kind == kUnitPositive)) ok = v <= 1;
      if (!ok) {
        char msg[200];
        if (f.n > 1) snprintf(msg, sizeof(msg), "%s%s[%d]: %g is not finite", prefix, f.name, i, v);
        else snprintf(msg, sizeof(msg), "%s%s: %g must be finite%s%s", prefix, f.name, v, f.kind == kFinite ? "" : " and ", f.kind == kFinite ? "" : want[f.kind]);
        err = msg;
        return false;
      }
    }
  return true;
}

#ifdef RG_POLICY_ABI_VERSION
// what rg_policy_create and rg_ppo_create check alike of an rg_policy_config (where rg_policy.h has been included): the
// version, the dimensions, both width lists and obs_clip.  The fields only the acting side reads are the caller's.
inline bool check_policy_config(const char *prefix, const rg_policy_config *cfg, std::string &err) {
  if (!check_abi(prefix, cfg->abi_version, RG_POLICY_ABI_VERSION, err)) return false;
  if (!check_reserved(prefix, "reserved0", cfg->reserved0, err)) return false;
  const IntField ints[] = {{"obs_dim", cfg->obs_dim, 1, RG_POLICY_MAX_OBS}, {"act_dim", cfg->act_dim, 1, RG_POLICY_MAX_ACT},
                           {"n_policy_layers", cfg->n_policy_layers, 0, RG_POLICY_MAX_LAYERS}, {"n_value_layers", cfg->n_value_layers, 0, RG_POLICY_MAX_LAYERS}};
  const RealField reals[] = {{"obs_clip", &cfg->obs_clip, 1, kNonNegative}};
  return check_ints(prefix, ints, err) &&
         check_widths(prefix, "policy_layers", cfg->policy_layers, cfg->n_policy_layers, RG_POLICY_MAX_LAYERS, RG_POLICY_MAX_WIDTH, err) &&
         check_widths(prefix, "value_layers", cfg->value_layers, cfg->n_value_layers, RG_POLICY_MAX_LAYERS, RG_POLICY_MAX_WIDTH, err) &&
         check_reals(prefix, reals, err);
}
#endif

#ifdef RG_RNN_ABI_VERSION
// what the acting side and the update check alike of an rg_rnn_config (where rg_rnn.h has been included): every field
inline bool check_rnn_config(const char *prefix, const rg_rnn_config *cfg, std::string &err) {
  if (!check_abi(prefix, cfg->abi_version, RG_RNN_ABI_VERSION, err)) return false;
  if (!check_reserved(prefix, "reserved0", cfg->reserved0, err)) return false;
  const IntField ints[] = {{"obs_dim", cfg->obs_dim, 1, RG_RNN_MAX_OBS}, {"act_dim", cfg->act_dim, 1, RG_RNN_MAX_ACT},
                           {"n_policy_layers", cfg->n_policy_layers, 0, RG_RNN_MAX_DENSE}, {"gru_units", cfg->gru_units, 1, RG_RNN_MAX_UNITS},
                           {"n_value_layers", cfg->n_value_layers, 0, RG_RNN_MAX_VALUE_LAYERS}};
  const RealField reals[] = {{"obs_clip", &cfg->obs_clip, 1, kNonNegative}};
  return check_ints(prefix, ints, err) &&
         check_widths(prefix, "policy_layers", cfg->policy_layers, cfg->n_policy_layers, RG_RNN_MAX_DENSE, RG_RNN_MAX_WIDTH, err) &&
         check_widths(prefix, "value_layers", cfg->value_layers, cfg->n_value_layers, RG_RNN_MAX_VALUE_LAYERS, RG_RNN_MAX_WIDTH, err) &&
         check_reals(prefix, reals, err);
}

// the parameter layout rule of rg_rnn.h
inline void fill_layout(const rg_rnn_config *cfg, rg_rnn_layout &L) {
  L = rg_rnn_layout{};
  const int H = cfg->gru_units, nd = cfg->n_policy_layers;
  int off = 0, prev = cfg->obs_dim;
  for (int l = 0; l < nd; l++) {
    const int width = cfg->policy_layers[l];
    L.dense_in[l] = prev; L.dense_out[l] = width;
    L.dense_w[l] = off; off += prev * width;
    L.dense_b[l] = off; off += width;
    prev = width;
  }
  L.n_dense = nd; L.n_x = prev; L.gru_units = H;
  L.w_ru = off; off += (prev + H) * 2 * H;
  L.b_ru = off; off += 2 * H;
  L.w_c = off; off += (prev + H) * H;
  L.b_c = off; off += H;
  L.head_w = off; off += H * cfg->act_dim;
  L.head_b = off; off += cfg->act_dim;
  L.logstd_offset = off;
  L.policy_count = off + cfg->act_dim;
  L.n_value = cfg->n_value_layers + 1;
  L.value_count = layer_layout(cfg->obs_dim, cfg->value_layers, cfg->n_value_layers, 1, L.value_in, L.value_out, L.value_w, L.value_b);
}

// the policy buffer's layout into the fields a kernel's descriptor D names as the tick's device code reads them
template <typename D>
void layout_to_dev(const rg_rnn_layout &L, D &d) {
  d.H = L.gru_units; d.n_dense = L.n_dense; d.n_x = L.n_x;
  for (int l = 0; l < 2; l++) { d.dense_in[l] = L.dense_in[l]; d.dense_out[l] = L.dense_out[l]; d.dense_w[l] = L.dense_w[l]; d.dense_b[l] = L.dense_b[l]; }
  d.w_ru = L.w_ru; d.b_ru = L.b_ru; d.w_c = L.w_c; d.b_c = L.b_c; d.head_w = L.head_w; d.head_b = L.head_b; d.logstd_off = L.logstd_offset;
}
#endif

#ifdef RG_PPO_ABI_VERSION
// an rg_ppo_config (where rg_ppo.h has been included): every update that takes one checks it alike
inline bool check_ppo_config(const rg_ppo_config *cfg, std::string &err) {
  const IntField ints[] = {{"epochs_policy", cfg->epochs_policy, 0, RG_PPO_MAX_EPOCHS}, {"epochs_value", cfg->epochs_value, 0, RG_PPO_MAX_EPOCHS},
                           {"conv_logpdf", cfg->conv_logpdf, RG_PPO_LOGPDF_EXACT, RG_PPO_LOGPDF_REFERENCE}};
  const RealField reals[] = {{"policy_lr", &cfg->policy_lr, 1, kNonNegative}, {"value_lr", &cfg->value_lr, 1, kNonNegative}, {"beta1", &cfg->beta1, 1, kBelowOne},
                             {"beta2", &cfg->beta2, 1, kBelowOne}, {"adam_eps", &cfg->adam_eps, 1, kPositive}, {"kl_target", &cfg->kl_target, 1, kPositive},
                             {"kl_cutoff_factor", &cfg->kl_cutoff_factor, 1, kNonNegative}, {"kl_cutoff_coef", &cfg->kl_cutoff_coef, 1, kNonNegative}};
  return check_abi("ppo_cfg.", cfg->abi_version, RG_PPO_ABI_VERSION, err) && check_ints("ppo_cfg.", ints, err) && check_reals("ppo_cfg.", reals, err);
}

// the samples of a rollout, T and B each within their own range: every update's create checks the product alike
inline bool check_samples(int T, int B, std::string &err) {
  if ((long long)T * B <= RG_PPO_MAX_SAMPLES) return true;
  char msg[128];
  snprintf(msg, sizeof(msg), "T * B: %lld above %d", (long long)T * B, RG_PPO_MAX_SAMPLES);
  err = msg;
  return false;
}
#endif

// ---- errors: h->err and the status of the caller's API ----------------------------------------------------------------------

template <typename H>
int hip_fail(H *h, int status, const char *what, hipError_t e) {
  h->err = std::string(what) + ": " + hipGetErrorString(e);
  return status;
}

// api: "RG_POLICY", "RG_GOTO", ...
template <typename H>
int no_device(H *h, int status, const char *api) {
  h->err = std::string("host-only handle (") + api + "_DEVICE_NONE): the arguments are valid, there is no device to run on";
  return status;
}

// 0, every API's OK, where the launch before went through
template <typename H>
int launch_status(H *h, int status, const char *what) {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? hip_fail(h, status, what, e) : 0;
}

template <typename H>
int null_arg(H *h, int status, const char *call, const char *name) {
  h->err = std::string(call) + ": null " + name;
  return status;
}

// in a function whose handle is h and whose file gives null_arg(h, call, name)
#define RG_NEED(call, ptr, name) \
  do { if (!(ptr)) return null_arg(h, call, name); } while (0)

}  // namespace
