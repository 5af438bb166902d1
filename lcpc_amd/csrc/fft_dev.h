// lcpc_amd/csrc/fft_dev.h -- the pass of the whole-vector transforms, once: its arguments, LDS layout, table look-up and body
// (pass_body, which K12's fft_pass_kernel in fft.hip and K14's dom_pass_kernel in domain.hip wrap), the launch of one pass and the
// walk over a plan's passes that launch_fft, launch_coset_fft and launch_extend run (run_passes).
//
// A transform of n = 2^log_n points is cut into passes by fft_plan.  Pass (t0, s) works on the sub-transforms of 2^(log_n - t0)
// points that the passes before it left behind: with r = log_n - t0 - s an element's index is (top, m, low) -- t0 + vector bits,
// s bits, r bits -- and the pass runs the 2^s-point transform over m for every (top, low), a "column".  In decimation in frequency
// (natural in, bit-reversed out) that is s radix-2 stages (a + b, (a - b) v^e) with the twiddles of the 2^s-point transform alone,
// followed by ONE multiplication per element with the twist v^((low * rev_s(m)) << t0); the last pass (r == 0) has no twist.
// Decimation in time (bit-reversed in, natural out) is the same network backwards: the passes from the last to the first, in each the
// twist first and then the stages (a + b v^e, a - b v^e) from the shortest distance to the longest.  Every pass reads and writes the
// same places, so a transform runs in place; the first pass may read another buffer.  The inverse forms run the same passes with
// v = w^-1 and multiply by n^-1 in the store of the last pass.
//
// A workgroup holds 2^log_c columns, 2^(s + log_c) elements, in LDS, one 32-bit limb plane after the other (lanes that walk
// consecutive elements hit consecutive banks).  Adjacent columns are adjacent in memory: a global access of the workgroup is a run
// of min(2^log_c, 2^r) * (r < log_c ? 2^s : 1) contiguous elements per row, never one lane per stride.  The vector index and the t0
// top bits are one number (vectors lie n apart), so n_vecs only lengthens the column list; columns past its end are masked.
// Twiddles: the 2^(s-1) twiddles of the 2^s-point transform are built in LDS by every workgroup from the two-level table
// (one multiplication each), the twist is one more product of two table entries.  All arithmetic is field_dev.h's fe_mul / fe_add /
// fe_sub on fully reduced elements, so every intermediate and every stored element is fully reduced.  All element indices are 64-bit.
#pragma once
#include <initializer_list>
#include <type_traits>

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

// The four modes of a pass.  PASS_PLAIN is K12's (include/lcpc_hip_fft.h): the twiddle table is that of 2^log_n points, and the store
// multiplies by n^-1 under a.scale.  The other three are K14's (include/lcpc_hip_domain.h).  A power t^j of the shift, j the NATURAL
// index of an element whatever the order it is stored in, comes from a two-level table like the twiddles': stab[i] = t^i for
// i < 2^hs, stab[2^hs + i] = t^(i 2^hs) (times n^-1 in the inverse direction, which then costs no multiply of its own).
//   DOM_LOAD   the pass that reads the input of a forward transform: every element times t^j as it is loaded.  The extension runs
//              2^b transforms per source vector: output vector V reads source vector V >> b, whose vectors lie 2^src_log apart and
//              read as zero from n_coeffs on, and its shift is t w_m^rev_b(V mod 2^b) -- the second factor from the twiddle table.
//   DOM_STORE  the pass that writes the output of an inverse transform: every element times t^j n^-1 as it is stored.
//   DOM_MID    every other pass of a K14 transform.
// In these three a.scale is unused and the twiddle table is that of 2^(log_n + tw_shift) points (the extension's: w_n = w_m^(2^b)):
// every exponent of the pass is shifted by tw_shift, which PASS_PLAIN knows to be zero at compile time.
enum : int { PASS_PLAIN = 0, DOM_LOAD = 1, DOM_STORE = 2, DOM_MID = 3 };
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

// one pass, whole: tile load, twist, s stages, twist, store.  d is read in the DOM_ modes only, n_inv in PASS_PLAIN only
template <int NL, int MODE>
LCPC_DEV void pass_body(const FftPass a, const DomPass d, const Fe<NL> n_inv) {
  extern __shared__ __attribute__((aligned(16))) u32 lds[];
  const u32 s = a.s, r = a.log_n - a.t0 - a.s, lc = a.log_c;
  const u32 rows = 1u << s, T = rows << lc, half = rows >> 1;
  u32* tile = lds;                       // [NL][T], element (m, col) at tile_at(m, col, lc)
  u32* tw = lds + (size_t)NL * T;        // [NL][half]: v^(i << (log_n - s))
  const u32 tid = threadIdx.x, nt = blockDim.x;
  const u64 q0 = (u64)blockIdx.x << lc;
  // how a tile element number e is read as (column, row) for the global accesses: the low min(lc, r) column bits vary fastest, then
  // the row, then the remaining column bits -- consecutive lanes take consecutive addresses as far as the layout has them
  const u32 lcl = lc < r ? lc : r;
  const u64 low_mask = ((u64)1 << r) - 1;
  const u32 tsh = MODE == PASS_PLAIN ? 0 : d.tw_shift;
  const u64 in_vec = ((u64)1 << a.log_n) - 1;

  for (u32 i = tid; i < half; i += nt) lds_put<NL>(tw, half, i, tab_pow<NL>(a.tab, a.h, ((u64)i << (a.log_n - s)) << tsh));

  for (u32 e = tid; e < T; e += nt) {
    const u32 cl = e & ((1u << lcl) - 1), m = (e >> lcl) & (rows - 1), ct = e >> (lcl + s);
    const u32 col = (ct << lcl) | cl;
    const u64 q = q0 + col;
    if (q < a.n_cols) {
      const u64 top = q >> r, low = q & low_mask;
      const u64 g = (top << (s + r)) + ((u64)m << r) + low;
      Fe<NL> v;
      if constexpr (MODE == DOM_LOAD) {
        const u64 vec = g >> a.log_n, i = g & in_vec;
        const u64 j = a.dit ? __brevll(i) >> (64 - a.log_n) : i;
        if (j < d.n_coeffs) {
          v = fe_load<NL>(a.src + (((vec >> d.b) << d.src_log) + i) * NL);
          Fe<NL> sc = tab_pow<NL>(d.stab, d.hs, j);
          if (d.b) sc = fe_mul<NL>(sc, tab_pow<NL>(a.tab, a.h, (u64)(__brev((u32)vec & ((1u << d.b) - 1)) >> (32 - d.b)) * j));
          v = fe_mul<NL>(v, sc);
        } else {
#pragma unroll
          for (int l = 0; l < NL; l++) v.v[l] = 0;
        }
      } else {
        v = fe_load<NL>(a.src + g * NL);
      }
      if (a.dit && r) v = fe_mul<NL>(v, tab_pow<NL>(a.tab, a.h, ((low * (u64)(__brev(m) >> (32 - s))) << a.t0) << tsh));
      lds_put<NL>(tile, T, tile_at(m, col, lc), v);
    }
  }
  __syncthreads();

  for (u32 k = 0; k < s; k++) {
    const u32 u = a.dit ? s - 1 - k : k;         // stage u pairs rows 2^(s - 1 - u) apart
    const u32 lhw = s - 1 - u;
    for (u32 b = tid; b < (T >> 1); b += nt) {
      const u32 col = b & ((1u << lc) - 1), pb = b >> lc;
      const u32 jl = pb & ((1u << lhw) - 1);
      const u32 i0 = ((pb >> lhw) << (lhw + 1)) | jl;
      const u32 e0 = tile_at(i0, col, lc), e1 = tile_at(i0 + (1u << lhw), col, lc);
      const Fe<NL> x = lds_get<NL>(tile, T, e0);
      Fe<NL> y = lds_get<NL>(tile, T, e1);
      if (lhw == 0) {                            // neighbouring rows: every twiddle of the stage is v^0 (uniform: no multiply)
        lds_put<NL>(tile, T, e0, fe_add<NL>(x, y));
        lds_put<NL>(tile, T, e1, fe_sub<NL>(x, y));
      } else if (a.dit) {
        y = fe_mul<NL>(y, lds_get<NL>(tw, half, jl << u));
        lds_put<NL>(tile, T, e0, fe_add<NL>(x, y));
        lds_put<NL>(tile, T, e1, fe_sub<NL>(x, y));
      } else {
        lds_put<NL>(tile, T, e0, fe_add<NL>(x, y));
        lds_put<NL>(tile, T, e1, fe_mul<NL>(fe_sub<NL>(x, y), lds_get<NL>(tw, half, jl << u)));
      }
    }
    __syncthreads();
  }

  for (u32 e = tid; e < T; e += nt) {
    const u32 cl = e & ((1u << lcl) - 1), m = (e >> lcl) & (rows - 1), ct = e >> (lcl + s);
    const u32 col = (ct << lcl) | cl;
    const u64 q = q0 + col;
    if (q < a.n_cols) {
      const u64 top = q >> r, low = q & low_mask;
      const u64 g = (top << (s + r)) + ((u64)m << r) + low;
      Fe<NL> v = lds_get<NL>(tile, T, tile_at(m, col, lc));
      if (!a.dit && r) v = fe_mul<NL>(v, tab_pow<NL>(a.tab, a.h, ((low * (u64)(__brev(m) >> (32 - s))) << a.t0) << tsh));
      if constexpr (MODE == DOM_STORE) {
        const u64 i = g & in_vec;
        v = fe_mul<NL>(v, tab_pow<NL>(d.stab, d.hs, a.dit ? i : __brevll(i) >> (64 - a.log_n)));
      }
      if constexpr (MODE == PASS_PLAIN) {
        if (a.scale) v = fe_mul<NL>(v, n_inv);
      }
      fe_store<NL>(a.dst + g * NL, v);
    }
  }
}

template <int NL> Fe<NL> fe_arg(const u32* w) {
  Fe<NL> r;
  for (int i = 0; i < NL; i++) r.v[i] = w ? w[i] : 0;
  return r;
}
// f(std::integral_constant<int, NL>) for the element width nl (nl_ok)
template <class F> hipError_t with_nl(int nl, F&& f) {
  switch (nl) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 6: return f(std::integral_constant<int, 6>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

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
// one pass on `st`: kernel is fft_pass_kernel<NL> or dom_pass_kernel<NL, MODE>, rest its second argument
template <int NL, class Rest>
hipError_t pass_launch(void (*kernel)(FftPass, Rest), const FftPass& a, const Rest& rest, hipStream_t st) {
  const size_t lds_bytes = pass_lds_bytes(NL, a);
  // (idempotent and cheap; set on every launch rather than cached in an unsynchronised static)
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3((unsigned)pass_blocks(a)), dim3(pass_lanes(a)), lds_bytes, st, a, rest);
  return hipGetLastError();
}

inline bool words_overlap(const uint32_t* a, uint64_t na, const uint32_t* b, uint64_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb * 4 && y < x + na * 4;
}

// What the three launchers run: the plan fft_plan(log_n, log_tile) over n_vecs vectors of 2^log_n elements in `out`.
struct FftRun {
  int nl;
  uint32_t log_n, log_tile;
  uint32_t log_tab;        // the twiddle table is that of 2^log_tab points (log_n, or the extension's log_m)
  uint64_t n_vecs;         // 1 .. 65535, the extension's blocks included
  bool dit;                // the plan from its last pass to its first
  int rev;                 // K13: < 0 from in to out before the passes, > 0 in place on the output's 2^log_tab-point vectors after them
  const uint32_t* in;      // read by the first launch only: in_elems elements (0: as many as the output), which must not meet
  uint64_t in_elems;       // the output --
  bool in_place;           // -- unless this is set and in == out
  uint32_t* out;
  const uint32_t* tab;     // a.tab of every pass
  hipStream_t st;
  uint32_t* n_launches;    // may be null
};
// a transform in one of the six forms (launch_fft, launch_coset_fft): in place or between disjoint ranges, K13 first for the II forms
inline FftRun form_run(int nl, int form, uint32_t log_n, uint32_t log_tile, uint32_t n_vecs, const uint32_t* in, uint32_t* out,
                       const uint32_t* tab, hipStream_t st, uint32_t* n_launches) {
  FftRun f;
  f.nl = nl; f.log_n = f.log_tab = log_n; f.log_tile = log_tile; f.n_vecs = n_vecs;
  f.dit = form != FFT_FFT_IO && form != FFT_IFFT_IO;
  f.rev = form == FFT_FFT_II || form == FFT_IFFT_II ? -1 : 0;
  f.in = in; f.in_elems = 0; f.in_place = true; f.out = out; f.tab = tab; f.st = st; f.n_launches = n_launches;
  return f;
}
// Every refusal the launchers share (hipErrorInvalidValue before any launch), the one-point copy, K13, and the passes in order:
// pass(k, n_pass, a) launches the k-th pass to run, a filled but for a.scale (0).  tabs: the device tables the passes read (f.tab
// among them), required where there is more than one point.
template <class Pass>
hipError_t run_passes(const FftRun& f, std::initializer_list<const uint32_t*> tabs, Pass&& pass) {
  uint32_t s[FFT_MAX_PASSES];
  const int n_pass = fft_plan(f.log_n, f.log_tile, s);
  if (!nl_ok(f.nl) || n_pass < 0 || f.n_vecs == 0 || f.n_vecs > 65535) return hipErrorInvalidValue;
  if (!f.in || !f.out || !elem_aligned(f.in, f.nl) || !elem_aligned(f.out, f.nl)) return hipErrorInvalidValue;
  for (const uint32_t* t : tabs)
    if (f.log_tab && (!t || !elem_aligned(t, f.nl))) return hipErrorInvalidValue;
  const uint64_t total = f.n_vecs << f.log_n;                       // (n_vecs < 2^16, log_n <= 32: no overflow)
  if (total >= ((uint64_t)1 << 39)) return hipErrorInvalidValue;    // K13's grid; a pass has at most total / 2 columns, 2^31 workgroups
  if (!(f.in_place && f.in == f.out) && words_overlap(f.in, (f.in_elems ? f.in_elems : total) * f.nl, f.out, total * f.nl)) return hipErrorInvalidValue;
  if (f.n_launches) *f.n_launches = 0;
  if (f.log_n == 0) {                                               // one point: the value itself (log_tab is 0 as well)
    if (f.in == f.out) return hipSuccess;
    return hipMemcpyAsync(f.out, f.in, (size_t)total * f.nl * 4, hipMemcpyDeviceToDevice, f.st);
  }
  uint32_t launches = 0;
  const uint32_t* src = f.in;
  if (f.rev < 0) {
    hipError_t e = launch_fft_bitrev(f.nl, f.in, f.out, f.log_n, total, f.st);
    if (e != hipSuccess) return e;
    launches++;
    src = f.out;
  }
  uint32_t t0s[FFT_MAX_PASSES], t0 = 0;
  for (int p = 0; p < n_pass; p++) { t0s[p] = t0; t0 += s[p]; }
  for (int k = 0; k < n_pass; k++) {
    const int p = f.dit ? n_pass - 1 - k : k;
    FftPass a;
    a.src = src; a.dst = f.out; a.tab = f.tab;
    a.log_n = f.log_n; a.t0 = t0s[p]; a.s = s[p]; a.h = fft_tab_split(f.log_tab);
    a.log_c = log_cols(f.nl, s[p]);
    a.n_cols = f.n_vecs << (f.log_n - s[p]);
    a.dit = f.dit; a.scale = 0;
    hipError_t e = pass(k, n_pass, a);
    if (e != hipSuccess) return e;
    launches++;
    src = f.out;
  }
  if (f.rev > 0) {
    hipError_t e = launch_fft_bitrev(f.nl, f.out, f.out, f.log_tab, total, f.st);
    if (e != hipSuccess) return e;
    launches++;
  }
  if (f.n_launches) *f.n_launches = launches;
  return hipSuccess;
}

}  // namespace
}  // namespace lcpc
