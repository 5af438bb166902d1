// lcpc_amd/csrc/quot.hip -- K15: batch inversion and pointwise arithmetic on element vectors; K16: division of columns of values on a
// domain by X - z or by X^n - 1 (include/lcpc_hip_quot.h).
//
// An inverse is a^(p - 2): about 1.4 multiplies per bit of p with the two-bit window used here, E = 357 for Ft255.  Montgomery's trick
// turns t inverses into one inverse and 3 (t - 1) multiplies -- but on a SIMD machine the one inverse is only cheap when the OTHER
// lanes of the wave that runs it do useful work too: an exponentiation executed "uniformly" by a wave costs its 64 lanes the issue
// slots of 64 different exponentiations, exactly what one inversion per lane costs.  So a tile is inverted in two levels, and the
// exponentiations of a tile are gathered into one full wave:
//   1. A workgroup of W waves (QT_LANES = 64 W lanes) owns a tile of QT_LANES * QT_C elements.  Lane l takes the elements
//      base + j QT_LANES + l (j < QT_C), so loads coalesce, and keeps their running products in registers, a zero replaced by one
//      (QT_C multiplies).
//   2. Every lane puts its total into LDS.  The QT_LANES totals go to the 64 lanes of wave 0, W each: a lane multiplies its totals
//      up, inverts the product -- 64 DIFFERENT exponentiations in one wave, so a tile pays the issue slots of one exponentiation per
//      QT_LANES * QT_C elements -- and back-substitutes into the inverse of every lane total (LDS again).  The exponent is the
//      compile-time p - 2 of the field, scanned by a loop whose branches depend on the exponent alone.
//   3. Every lane fetches the inverse of its total and back-substitutes its QT_C elements (2 multiplies each), reading the element a
//      second time instead of holding it in registers across the barrier.  A zero stores zero; positions past the end act as ones and
//      store nothing.
// Multiplies per element, counted as wave instructions per 64 elements: 3 + (3 (W - 1) + E) / (W QT_C).  While wave 0 runs step 2 the
// other waves of the workgroup wait, so the step only costs its issue slots when OTHER workgroups fill the CU meanwhile: the chain of
// a tile is QT_C + 3 (W - 1) + E + 2 QT_C multiplies long and a CU finishes k tiles per chain with k resident workgroups.  The
// running products take QT_C NL registers, which sets k: Ft63 and Ft127 (62 and 98 VGPRs) run W = 8 with four and two workgroups per
// CU; Ft191 and Ft255 (146 and 148 VGPRs, three waves per SIMD) run W = 4, three workgroups per CU, where W = 8 leaves room for one
// and measured 1.47 times slower (DESIGN section 4 has the count and section 6 the figures).  No instantiation uses scratch.
// DIV is the same tile over b with one more multiply by a.  ADD, SUB and MUL are one element per lane.
//
// K16 is the same tile with generated denominators: position q of a vector holds the value at x_k = shift w_m^k, k = q or rev_m(q), and
// the denominator is x_k - z, or shift^n w_m^(k n mod m) - 1, with w_m^e from the forward twiddle table of m points (two loads and a
// multiply) -- computed again in step 3, not held.  After the tile's inverses exist the lane walks the n_vecs vectors at its
// positions: load, subtract y_v (X - z only), multiply, store.  The inversion is paid per position, not per value.
#include <utility>

#include "fft_dev.h"

namespace lcpc {

namespace {

// f(0), f(1), ... with the index a compile-time constant: the bodies below hold several inlined multiplies, too much for the unroller's
// budget, and a loop left rolled would put the register arrays into scratch
template <class F, int... J> LCPC_DEV void static_for(F&& f, std::integer_sequence<int, J...>) { (f(std::integral_constant<int, J>{}), ...); }

// QT_C elements per lane; lanes per workgroup by field (the comment at the top says why), QT_W waves
constexpr int QT_C = 8;
template <int NL> constexpr int QT_LANES = NL >= 6 ? 256 : 512;
template <int NL> constexpr u32 QT_W = QT_LANES<NL> / 64;

template <int NL> LCPC_DEV bool fe_is_zero(const Fe<NL>& a) {
  u32 x = 0;
#pragma unroll
  for (int l = 0; l < NL; l++) x |= a.v[l];
  return x == 0;
}
template <int NL> LCPC_DEV Fe<NL> fe_pick(bool c, const Fe<NL>& a, const Fe<NL>& b) {
  Fe<NL> r;
#pragma unroll
  for (int l = 0; l < NL; l++) r.v[l] = c ? a.v[l] : b.v[l];
  return r;
}

// word i of p - 2 (p = 1 mod 2^32 and word 1 of p is not zero: one borrow)
template <int NL> LCPC_DEV u32 pm2_word(u32 i) {
  u32 w = 0xffffffffu;
#pragma unroll
  for (int l = 1; l < NL; l++) w = i == (u32)l ? Mod<NL>::P[l] - (l == 1 ? 1u : 0u) : w;
  return w;
}

// a^(p - 2), a != 0: two-bit digits of the exponent from the top; every branch depends on the exponent alone
template <int NL> LCPC_DEV Fe<NL> fe_inv(const Fe<NL>& a, const Fe<NL>& one) {
  const Fe<NL> a2 = fe_mul<NL>(a, a), a3 = fe_mul<NL>(a2, a);
  Fe<NL> acc = one;
#pragma unroll 1
  for (int i = 16 * NL - 1; i >= 0; i--) {
    const u32 d = (pm2_word<NL>((u32)i >> 4) >> (2 * (i & 15))) & 3u;
    acc = fe_mul<NL>(acc, acc);
    acc = fe_mul<NL>(acc, acc);
    if (d) acc = fe_mul<NL>(acc, fe_pick<NL>(d == 1, a, fe_pick<NL>(d == 2, a2, a3)));
  }
  return acc;
}

// The tile of one workgroup.  den(j): the lane's j-th element (anything for a position past the end: fin ignores it), called twice;
// fin(j, r): r = the inverse of that element, zero for a zero.  lds: 2 * QT_LANES<NL> * NL words
template <int NL, class Den, class Fin> LCPC_DEV void inverse_tile(u32* lds, const Fe<NL>& one, Den den, Fin fin) {
  u32* tot = lds;                          // [NL][QT_LANES<NL>]: lane totals, then their inverses
  u32* exc = lds + (size_t)NL * QT_LANES<NL>;  // [NL][QT_LANES<NL>]: wave 0's exclusive prefixes
  const u32 tid = threadIdx.x;
  Fe<NL> pre[QT_C];
  static_for([&](auto jc) {
    constexpr int j = jc;
    Fe<NL> x = den(j);
    x = fe_pick<NL>(fe_is_zero<NL>(x), one, x);
    if constexpr (j > 0) pre[j] = fe_mul<NL>(pre[j - 1], x);
    else pre[j] = x;
  }, std::make_integer_sequence<int, QT_C>{});
  lds_put<NL>(tot, QT_LANES<NL>, tid, pre[QT_C - 1]);
  __syncthreads();
  if (tid < 64) {
    Fe<NL> run = lds_get<NL>(tot, QT_LANES<NL>, tid);
#pragma unroll 1
    for (u32 k = 1; k < QT_W<NL>; k++) {
      lds_put<NL>(exc, QT_LANES<NL>, k * 64 + tid, run);
      run = fe_mul<NL>(run, lds_get<NL>(tot, QT_LANES<NL>, k * 64 + tid));
    }
    Fe<NL> inv = fe_inv<NL>(run, one);
#pragma unroll 1
    for (u32 k = QT_W<NL> - 1; k >= 1; k--) {
      const Fe<NL> t = lds_get<NL>(tot, QT_LANES<NL>, k * 64 + tid);
      lds_put<NL>(tot, QT_LANES<NL>, k * 64 + tid, fe_mul<NL>(inv, lds_get<NL>(exc, QT_LANES<NL>, k * 64 + tid)));
      inv = fe_mul<NL>(inv, t);
    }
    lds_put<NL>(tot, QT_LANES<NL>, tid, inv);
  }
  __syncthreads();
  Fe<NL> inv = lds_get<NL>(tot, QT_LANES<NL>, tid);
  static_for([&](auto jc) {
    constexpr int j = QT_C - 1 - jc;
    Fe<NL> x = den(j);
    const bool z = fe_is_zero<NL>(x);
    Fe<NL> r = inv;
    if constexpr (j > 0) {
      r = fe_mul<NL>(inv, pre[j - 1]);
      inv = fe_mul<NL>(inv, fe_pick<NL>(z, one, x));
    }
    fin(j, fe_pick<NL>(z, fe_zero<NL>(), r));
  }, std::make_integer_sequence<int, QT_C>{});
}

template <int NL> struct InvArgs {
  const u32* a;        // DIV only
  const u32* b;        // the elements to invert
  u32* out;
  u64 n;
  Fe<NL> one;
};

template <int NL, bool DIV> __global__ void __launch_bounds__(QT_LANES<NL>) inverse_kernel(InvArgs<NL> p) {
  __shared__ __attribute__((aligned(16))) u32 lds[2 * QT_LANES<NL> * NL];
  const u64 base = (u64)blockIdx.x * (QT_LANES<NL> * QT_C) + threadIdx.x;
  inverse_tile<NL>(
      lds, p.one,
      [&](int j) {
        const u64 i = base + (u64)j * QT_LANES<NL>;
        return i < p.n ? fe_load<NL>(p.b + i * NL) : fe_zero<NL>();
      },
      [&](int j, const Fe<NL>& r) {
        const u64 i = base + (u64)j * QT_LANES<NL>;
        if (i < p.n) {
          if constexpr (DIV) fe_store<NL>(p.out + i * NL, fe_mul<NL>(fe_load<NL>(p.a + i * NL), r));
          else fe_store<NL>(p.out + i * NL, r);
        }
      });
}

template <int NL, int OP> __global__ void __launch_bounds__(256) pointwise_kernel(const u32* a, const u32* b, u32* out, u64 n) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Fe<NL> x = fe_load<NL>(a + i * NL), y = fe_load<NL>(b + i * NL);
  fe_store<NL>(out + i * NL, OP == QUOT_ADD ? fe_add<NL>(x, y) : OP == QUOT_SUB ? fe_sub<NL>(x, y) : fe_mul<NL>(x, y));
}

template <int NL> struct DomQuotArgs {
  const u32* in;
  u32* out;
  const u32* tab;      // forward twiddle table of 2^log_m points; null for log_m == 0
  const u32* y;        // LINEAR: n_vecs elements
  u64 m;
  u32 log_m, log_n, h, n_vecs, bitrev;
  Fe<NL> one, shift, z;   // shift: the shift (LINEAR) or shift^n (VANISH)
};

template <int NL, int KIND> __global__ void __launch_bounds__(QT_LANES<NL>) dom_quot_kernel(DomQuotArgs<NL> p) {
  __shared__ __attribute__((aligned(16))) u32 lds[2 * QT_LANES<NL> * NL];
  const u64 base = (u64)blockIdx.x * (QT_LANES<NL> * QT_C) + threadIdx.x;
  inverse_tile<NL>(
      lds, p.one,
      [&](int j) {
        const u64 q = base + (u64)j * QT_LANES<NL>;
        if (q >= p.m) return fe_zero<NL>();
        Fe<NL> x = p.shift;
        if (p.log_m) {
          const u64 k = p.bitrev ? __brevll(q) >> (64 - p.log_m) : q;
          const u64 e = KIND == QUOT_LINEAR ? k : (k << p.log_n) & (p.m - 1);
          x = fe_mul<NL>(x, tab_pow<NL>(p.tab, p.h, e));
        }
        return fe_sub<NL>(x, KIND == QUOT_LINEAR ? p.z : p.one);
      },
      [&](int j, const Fe<NL>& r) {
        const u64 q = base + (u64)j * QT_LANES<NL>;
        if (q >= p.m) return;
#pragma unroll 1
        for (u32 v = 0; v < p.n_vecs; v++) {
          const u64 i = (u64)v * p.m + q;
          Fe<NL> x = fe_load<NL>(p.in + i * NL);
          if constexpr (KIND == QUOT_LINEAR) x = fe_sub<NL>(x, fe_load<NL>(p.y + (u64)v * NL));
          fe_store<NL>(p.out + i * NL, fe_mul<NL>(x, r));
        }
      });
}

// R = 2^(32 nl) mod p, the Montgomery form of one
template <int NL> Fe<NL> mont_one() {
  u32 r[NL] = {1};
  for (int bit = 0; bit < 32 * NL; bit++) {
    u32 top = r[NL - 1] >> 31;
    for (int l = NL - 1; l > 0; l--) r[l] = (r[l] << 1) | (r[l - 1] >> 31);
    r[0] <<= 1;
    bool ge = top != 0;
    if (!ge) {
      ge = true;
      for (int l = NL - 1; l >= 0; l--)
        if (r[l] != Mod<NL>::P[l]) { ge = r[l] > Mod<NL>::P[l]; break; }
    }
    if (ge) {
      u64 br = 0;
      for (int l = 0; l < NL; l++) {
        const u64 d = (u64)r[l] - Mod<NL>::P[l] - br;
        r[l] = (u32)d;
        br = (d >> 32) & 1;
      }
    }
  }
  Fe<NL> o;
  for (int l = 0; l < NL; l++) o.v[l] = r[l];
  return o;
}

inline bool words_meet(const uint32_t* a, uint64_t na, const uint32_t* b, uint64_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb * 4 && y < x + na * 4;
}
// an input and the output: the same range or disjoint ones
inline bool io_ok(const uint32_t* in, const uint32_t* out, uint64_t words) { return in == out || !words_meet(in, words, out, words); }

template <int NL> hipError_t inverse_nl(const uint32_t* a, const uint32_t* b, uint32_t* out, uint64_t n, hipStream_t st) {
  static_assert((u32)QT_LANES<NL> * QT_C == quot_tile(NL), "kernels.h states the tile");
  InvArgs<NL> p;
  p.a = a; p.b = b; p.out = out; p.n = n; p.one = mont_one<NL>();
  const unsigned blocks = (unsigned)((n + quot_tile(NL) - 1) / quot_tile(NL));      // (n < 2^39: below 2^27)
  if (a) hipLaunchKernelGGL((inverse_kernel<NL, true>), dim3(blocks), dim3(QT_LANES<NL>), 0, st, p);
  else hipLaunchKernelGGL((inverse_kernel<NL, false>), dim3(blocks), dim3(QT_LANES<NL>), 0, st, p);
  return hipGetLastError();
}

hipError_t inverse_any(int nl, const uint32_t* a, const uint32_t* b, uint32_t* out, uint64_t n, hipStream_t st) {
  switch (nl) {
    case 2: return inverse_nl<2>(a, b, out, n, st);
    case 4: return inverse_nl<4>(a, b, out, n, st);
    case 6: return inverse_nl<6>(a, b, out, n, st);
    default: return inverse_nl<8>(a, b, out, n, st);
  }
}

template <int NL> hipError_t pointwise_nl(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint64_t n, hipStream_t st) {
  const dim3 grid((unsigned)((n + 255) / 256)), lanes(256);                 // (n < 2^39: below 2^31)
  if (op == QUOT_ADD) hipLaunchKernelGGL((pointwise_kernel<NL, QUOT_ADD>), grid, lanes, 0, st, a, b, out, n);
  else if (op == QUOT_SUB) hipLaunchKernelGGL((pointwise_kernel<NL, QUOT_SUB>), grid, lanes, 0, st, a, b, out, n);
  else hipLaunchKernelGGL((pointwise_kernel<NL, QUOT_MUL>), grid, lanes, 0, st, a, b, out, n);
  return hipGetLastError();
}

template <int NL>
hipError_t dom_quot_nl(int kind, int bitrev, uint32_t log_m, uint32_t log_n, uint32_t n_vecs, const uint32_t* in, uint32_t* out, const uint32_t* tab_m,
                       const uint32_t* shift, const uint32_t* z, const uint32_t* y, hipStream_t st) {
  DomQuotArgs<NL> p;
  p.in = in; p.out = out; p.tab = tab_m; p.y = y;
  p.m = (uint64_t)1 << log_m; p.log_m = log_m; p.log_n = log_n; p.h = fft_tab_split(log_m); p.n_vecs = n_vecs; p.bitrev = bitrev ? 1 : 0;
  p.one = mont_one<NL>();
  p.shift = shift ? fe_arg<NL>(shift) : p.one;
  p.z = fe_arg<NL>(z);
  const unsigned blocks = (unsigned)((p.m + quot_tile(NL) - 1) / quot_tile(NL));
  if (kind == QUOT_LINEAR) hipLaunchKernelGGL((dom_quot_kernel<NL, QUOT_LINEAR>), dim3(blocks), dim3(QT_LANES<NL>), 0, st, p);
  else hipLaunchKernelGGL((dom_quot_kernel<NL, QUOT_VANISH>), dim3(blocks), dim3(QT_LANES<NL>), 0, st, p);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_batch_inverse(int nl, const uint32_t* in, uint32_t* out, uint64_t n, hipStream_t st) {
  if (!nl_ok(nl) || !in || !out || !elem_aligned(in, nl) || !elem_aligned(out, nl)) return hipErrorInvalidValue;
  if (n == 0 || n >= ((uint64_t)1 << 39) || !io_ok(in, out, n * nl)) return hipErrorInvalidValue;
  return inverse_any(nl, nullptr, in, out, n, st);
}

hipError_t launch_pointwise(int nl, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint64_t n, hipStream_t st) {
  if (!nl_ok(nl) || op < QUOT_ADD || op > QUOT_DIV || !a || !b || !out) return hipErrorInvalidValue;
  if (!elem_aligned(a, nl) || !elem_aligned(b, nl) || !elem_aligned(out, nl)) return hipErrorInvalidValue;
  if (n == 0 || n >= ((uint64_t)1 << 39) || !io_ok(a, out, n * nl) || !io_ok(b, out, n * nl)) return hipErrorInvalidValue;
  if (op == QUOT_DIV) return inverse_any(nl, a, b, out, n, st);
  switch (nl) {
    case 2: return pointwise_nl<2>(op, a, b, out, n, st);
    case 4: return pointwise_nl<4>(op, a, b, out, n, st);
    case 6: return pointwise_nl<6>(op, a, b, out, n, st);
    default: return pointwise_nl<8>(op, a, b, out, n, st);
  }
}

hipError_t launch_domain_quotient(int nl, int kind, int bitrev, uint32_t log_m, uint32_t log_n, uint32_t n_vecs, const uint32_t* in, uint32_t* out,
                                  const uint32_t* tab_m, const uint32_t* shift, const uint32_t* z, const uint32_t* y, hipStream_t st) {
  if (!nl_ok(nl) || (kind != QUOT_LINEAR && kind != QUOT_VANISH) || log_m > FFT_MAX_LOG_N || n_vecs == 0 || n_vecs > 65535) return hipErrorInvalidValue;
  if (!in || !out || !elem_aligned(in, nl) || !elem_aligned(out, nl)) return hipErrorInvalidValue;
  if (log_m && (!tab_m || !elem_aligned(tab_m, nl))) return hipErrorInvalidValue;
  if (kind == QUOT_LINEAR ? (!z || !y || !elem_aligned(y, nl)) : (!shift || log_n > log_m)) return hipErrorInvalidValue;
  const uint64_t total = (uint64_t)n_vecs << log_m;                 // (n_vecs < 2^16, log_m <= 32: no overflow)
  if (total >= ((uint64_t)1 << 39) || !io_ok(in, out, total * nl)) return hipErrorInvalidValue;
  if (kind == QUOT_LINEAR && words_meet(y, (uint64_t)n_vecs * nl, out, total * nl)) return hipErrorInvalidValue;
  if (kind == QUOT_VANISH) { z = nullptr; y = nullptr; }
  switch (nl) {
    case 2: return dom_quot_nl<2>(kind, bitrev, log_m, log_n, n_vecs, in, out, tab_m, shift, z, y, st);
    case 4: return dom_quot_nl<4>(kind, bitrev, log_m, log_n, n_vecs, in, out, tab_m, shift, z, y, st);
    case 6: return dom_quot_nl<6>(kind, bitrev, log_m, log_n, n_vecs, in, out, tab_m, shift, z, y, st);
    default: return dom_quot_nl<8>(kind, bitrev, log_m, log_n, n_vecs, in, out, tab_m, shift, z, y, st);
  }
}

}  // namespace lcpc
