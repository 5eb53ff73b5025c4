// rg_srb_ground.inc -- the ground function h(x, y; robot) of include/rg_srb.h, shared by rg_srb_terrain.hip and
// rg_srb_contact.hip.  Included inside the including file's anonymous namespace, after rg_srb_handle.h (rg_srb_ground) and
// under its `#pragma clang fp contract(off)`.  tests/terrain_model.py restates it operation for operation.

constexpr double kCoordBound = 1099511627776.0;   // 2^40: lattice coordinates are clamped to it before they become integers

#include "rg_stream_dev.inc"   // the chain over the three words (key, I, J)

// h(x, y; robot b) of rg_srb.h.  g.kind is RANDOM or GRID (wave-uniform).
struct Ground {
  rg_srb_ground g;
  __device__ __forceinline__ double operator()(int b, double x, double y) const {
    double s, t;
    if (g.kind == RG_SRB_TERRAIN_GRID) { s = (x - g.x0) / g.cell; t = (y - g.y0) / g.cell; }
    else { s = x / g.cell; t = y / g.cell; }
    s = fmin(fmax(s, -kCoordBound), kCoordBound);   // a NaN becomes the lower bound
    t = fmin(fmax(t, -kCoordBound), kCoordBound);
    const double fi = floor(s), fj = floor(t);
    const double u = s - fi, v = t - fj;
    const long long i = (long long)fi, j = (long long)fj;
    double h00, h10, h01, h11;
    if (g.kind == RG_SRB_TERRAIN_GRID) {
      const long long rm = g.rows - 1, cm = g.cols - 1;
      const size_t i0 = (size_t)(i < 0 ? 0 : (i > rm ? rm : i)), i1 = (size_t)(i + 1 < 0 ? 0 : (i + 1 > rm ? rm : i + 1));
      const size_t j0 = (size_t)(j < 0 ? 0 : (j > cm ? cm : j)), j1 = (size_t)(j + 1 < 0 ? 0 : (j + 1 > cm ? cm : j + 1));
      const size_t C = (size_t)g.cols;
      h00 = g.heights[i0 * C + j0]; h10 = g.heights[i1 * C + j0];
      h01 = g.heights[i0 * C + j1]; h11 = g.heights[i1 * C + j1];
    } else {
      const unsigned long long key = g.key ? (unsigned long long)g.key[b] : 0ull;
      const unsigned long long hk = mix_word(g.seed, key);
      const unsigned long long a0 = mix_word(hk, (unsigned long long)(i >> 1)), a1 = mix_word(hk, (unsigned long long)((i + 1) >> 1));
      const unsigned long long J0 = (unsigned long long)(j >> 1), J1 = (unsigned long long)((j + 1) >> 1);
      h00 = g.amplitude * unit53(mix_word(a0, J0)); h10 = g.amplitude * unit53(mix_word(a1, J0));
      h01 = g.amplitude * unit53(mix_word(a0, J1)); h11 = g.amplitude * unit53(mix_word(a1, J1));
    }
    if (u >= v) return h00 + u * (h10 - h00) + v * (h11 - h10);
    return h00 + u * (h11 - h01) + v * (h01 - h00);
  }
};
