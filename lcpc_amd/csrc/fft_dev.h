// lcpc_amd/csrc/fft_dev.h -- what the pass kernels of the whole-vector transforms share, K12 (fft.hip, which describes the pass) and
// K14 (domain.hip): the arguments of a pass, its LDS layout, the two-level table look-up and the launch geometry.
#pragma once
#include "kernels.h"
#include "field_dev.h"

namespace lcpc {
namespace {

struct FftPass {
  const u32* src;
  u32* dst;
  const u32* tab;      // two-level table of the direction's root
  u64 n_cols;          // n_vecs << (log_n - s)
  u32 log_n, t0, s, h, log_c;
  int dit, scale;
};

// K14 (include/lcpc_hip_domain.h).  A power t^j of the shift, j the NATURAL index of an element whatever the order it is stored in,
// comes from a two-level table like the twiddles': stab[i] = t^i for i < 2^hs, stab[2^hs + i] = t^(i 2^hs) (times n^-1 in the
// inverse direction, which then costs no multiply of its own).
//   DOM_LOAD   the pass that reads the input of a forward transform: every element times t^j as it is loaded.  The extension runs
//              2^b transforms per source vector: output vector V reads source vector V >> b, whose vectors lie 2^src_log apart and
//              read as zero from n_coeffs on, and its shift is t w_m^rev_b(V mod 2^b) -- the second factor from the twiddle table.
//   DOM_STORE  the pass that writes the output of an inverse transform: every element times t^j n^-1 as it is stored (a.scale unused).
//   DOM_MID    every other pass of a K14 transform: K12's pass.
// In all three the twiddle table is that of 2^(log_n + tw_shift) points (the extension's: w_n = w_m^(2^b)): every exponent of the
// pass is shifted by tw_shift.
enum : int { DOM_LOAD = 1, DOM_STORE = 2, DOM_MID = 3 };
struct DomPass {
  const u32* stab;
  u64 n_coeffs;
  u32 hs, b, src_log, tw_shift;
};

template <int NL> LCPC_DEV void lds_put(u32* base, u32 plane, u32 i, const Fe<NL>& v) {
#pragma unroll
  for (int l = 0; l < NL; l++) base[l * plane + i] = v.v[l];
}
template <int NL> LCPC_DEV Fe<NL> lds_get(const u32* base, u32 plane, u32 i) {
  Fe<NL> v;
#pragma unroll
  for (int l = 0; l < NL; l++) v.v[l] = base[l * plane + i];
  return v;
}
// where element (row m, column col) of a tile of 2^lc columns lies in a limb plane: the column is XORed with the row's low bits.  The
// stages walk a row's columns with consecutive lanes and the transposing loads and stores of a pass with fewer low bits than
// columns walk the rows of one column: both then hit different banks (unswizzled, the second is a stride of 2^lc words)
LCPC_DEV u32 tile_at(u32 m, u32 col, u32 lc) { return (m << lc) | (col ^ (m & ((1u << lc) - 1))); }
// v^e for e < 2^log_n from the two-level table
template <int NL> LCPC_DEV Fe<NL> tab_pow(const u32* tab, u32 h, u64 e) {
  const u64 lo = e & (((u64)1 << h) - 1), hi = e >> h;
  return fe_mul<NL>(fe_load<NL>(tab + lo * NL), fe_load<NL>(tab + (((u64)1 << h) + hi) * NL));
}

template <int NL> Fe<NL> fe_arg(const u32* w) {
  Fe<NL> r;
  for (int i = 0; i < NL; i++) r.v[i] = w ? w[i] : 0;
  return r;
}
inline bool nl_ok(int nl) { return nl == 2 || nl == 4 || nl == 6 || nl == 8; }
inline bool elem_aligned(const void* p, int nl) { return reinterpret_cast<uintptr_t>(p) % (nl % 4 == 0 ? 16 : 8) == 0; }

// the tile of a workgroup holds at most 64 KiB of elements (two workgroups per CU beside their twiddles) and at most 256 columns
inline uint32_t log_cols(int nl, uint32_t s) {
  uint32_t cap = 0;
  while (((size_t)8 * nl << cap) <= ((size_t)64 << 10)) cap++;      // largest cap with 4 nl 2^cap <= 64 KiB
  const uint32_t lc = cap - s;
  return lc < 8 ? lc : 8;
}
// LDS bytes, workgroups and lanes of a pass
inline size_t pass_lds_bytes(int nl, const FftPass& a) { return (((size_t)1 << (a.s + a.log_c)) + ((size_t)1 << (a.s - 1))) * nl * 4; }
inline uint64_t pass_blocks(const FftPass& a) { return (a.n_cols + (((uint64_t)1 << a.log_c) - 1)) >> a.log_c; }
inline unsigned pass_lanes(const FftPass& a) {
  const size_t nt = ((size_t)1 << (a.s + a.log_c)) / 2;
  return (unsigned)(nt < 64 ? 64 : nt > 1024 ? 1024 : nt);
}

}  // namespace
}  // namespace lcpc
