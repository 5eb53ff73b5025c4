// rg_stream_dev.inc -- the counter-based stream of include/rg_stream.h on the device, once: every unit that draws (the episode
// reset, the ground function, the agents' noise and sampler, the domain randomiser, the sensor model, the estimator model)
// includes this file.  Included inside the including file's anonymous namespace and after its `#pragma clang fp contract(off)`.
// Device functions and constants only, no kernel and no host code: what is not called is not emitted.  rg_mpc.hip does not
// include it, so the source hash behind profiles/ does not move.  tests/stream_model.py restates it in numpy.
#ifndef RG_STREAM_DEV_INC
#define RG_STREAM_DEV_INC

constexpr double kTickBound = 4503599627370496.0;   // 2^52: a tick row is clamped to it before it becomes an integer
constexpr double kRoot3 = 1.7320508075688772;

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// one round of the chain: h = seed, then h = mix_word(h, w) for every word in order
__device__ __forceinline__ unsigned long long mix_word(unsigned long long h, unsigned long long w) { return mix64((h ^ w) + 0x9E3779B97F4A7C15ull); }
// u
__device__ __forceinline__ double unit53(unsigned long long h) { return (double)(h >> 11) * 0x1.0p-53; }

// a state row's integer (key, draws, episode): through int64 to uint64
__device__ __forceinline__ unsigned long long word_of(double v) { return (unsigned long long)(long long)v; }
// a tick, delay or run row, which the caller may have written: clamped, a NaN is 0
__device__ __forceinline__ unsigned long long bounded(double v, double hi) { return (unsigned long long)fmin(fmax(v, 0.0), hi); }

// ix(k, row, 0)
__device__ __forceinline__ unsigned long long index_word(unsigned long long k, int row) { return (k << 12) | ((unsigned long long)row << 2); }

// n: hp = the chain up to and with the purpose, ix = ix(k, row, 0)
__device__ __forceinline__ double unit_noise(unsigned long long hp, unsigned long long ix) {
  const double u0 = unit53(mix_word(hp, ix)), u1 = unit53(mix_word(hp, ix | 1ull)), u2 = unit53(mix_word(hp, ix | 2ull)), u3 = unit53(mix_word(hp, ix | 3ull));
  return (((u0 + u1) + (u2 + u3)) - 2.0) * kRoot3;
}

// whether every purpose lies in the user's block of 16 (the registry of rg_stream.h): blocks do not overlap, so neither do users
template <typename... P>
constexpr bool purposes_in_block(int block, P... purpose) { return ((purpose / 16 == block) && ...); }

#endif
