// lcpc_amd/csrc/sumcheck.hip -- K18: the round sums of a sumcheck over a composition of tables; K19: the binding of a variable; K18f:
// both in one pass (include/lcpc_hip_sumcheck.h; the launchers' contracts are in kernels.h).
//
// K18.  A lane takes pairs in a grid-stride loop, one per stride, over at most max_groups workgroups of 256 lanes.  For a pair it walks
// the terms; for a term it loads (lo, hi) of every factor, forms hi - lo ONCE and reaches ext(., i, t) for t = 1, 2 ... d by repeated
// fe_add -- the points 0 ... d need no multiply --, multiplies the factors (n_factors - 1 multiplies per t) and adds the d + 1 products
// to the d + 1 sums of THAT term.  The sums are kept per term because the coefficient is applied to the finished sum, once per term
// and t (the sum is linear), not to every element.  A table that two terms share is loaded by both; the second load hits the cache.
// Every sum is a fully reduced element (fe_add), so a sum does not depend on how the pairs are spread over lanes and workgroups:
// field addition is exact and commutative, the limbs are the same for every grid.  The lanes' sums are folded across the wave by
// shuffles and across the four waves through LDS, as field_dot_kernel does; the workgroup stores one part per term and t.  A second
// launch of d + 1 workgroups (K18b) adds the parts, multiplies by c_m and adds the terms.  launch_field_sum adds parts as well, but
// it could not apply the coefficient or add the terms: that would be a third launch, so K18b is a kernel of its own.  A single workgroup
// finishes the sums itself: one launch.  No workgroup waits for another: no atomics, no spinning, no grid synchronisation.
//
// The term loop and the loop over t are unrolled over their limits with uniform guards (m < n_terms, t <= d) so that the
// MAX_TERMS x (MAX_FACTORS + 1) sums and the MAX_FACTORS + 1 running products are registers with constant indices; the factor loop is a
// run-time loop.  That is the only specialisation: per element width and order, no kernel per term shape.  DESIGN section 4 has the
// VGPR counts; no instantiation uses scratch.
//
// K19.  out[j][i] = lo + r (hi - lo): one multiply per output element, one element per lane, the table the grid's second dimension.
//
// K18f shares K18's body: lane i < n / 4 first binds, for every table, the two pairs whose results are pair i of the bound table --
// (i, i + n/2) and (i + n/4, i + 3n/4), or (4i, 4i + 1) and (4i + 2, 4i + 3) --, stores the two results, and then runs K18's walk on pair i
// of the BOUND tables, which it reads back from where it has just stored them (its own stores, in program order; no other lane
// writes them).  Keeping them in registers instead would take 2 x 8 tables x NL registers beside the sums.  Under HIGH_FIRST a lane
// writes only the places i and i + n/4 of a table, which it alone reads, so a table may be bound in place.
#include <utility>

#include "fft_dev.h"

namespace lcpc {

namespace {

template <class F, int... J> LCPC_DEV void static_for(F&& f, std::integer_sequence<int, J...>) { (f(std::integral_constant<int, J>{}), ...); }

constexpr int SM_T = (int)SUMCHECK_MAX_TERMS, SM_D1 = (int)SUMCHECK_MAX_FACTORS + 1, SM_W = (int)SUMCHECK_LANES / 64;

struct TermsArg {
  u32 n_terms, d;
  u32 n_factors[SM_T];
  u32 table[SM_T][SUMCHECK_MAX_FACTORS];
};
template <int NL> struct RoundArgs {
  const u32* tab[SUMCHECK_MAX_TABLES];   // K18: the tables; K18f: the inputs of the bind
  u32* out[SUMCHECK_MAX_TABLES];         // K18f: the bound tables
  u32 n_tables;
  TermsArg tm;
  u64 pairs;                             // the pairs of the round: n / 2; K18f: n / 4
  Fe<NL> r;                              // K18f
  Fe<NL> coeff[SM_T];                    // c_m (one where the caller gave none)
  u32* work;
  u32* evals;
};

template <int NL> LCPC_DEV Fe<NL> fe_shfl_down(const Fe<NL>& a, int d) {
  Fe<NL> r;
#pragma unroll
  for (int l = 0; l < NL; l++) r.v[l] = __shfl_down(a.v[l], d, 64);
  return r;
}
// lo + r (hi - lo)
template <int NL> LCPC_DEV Fe<NL> fe_bind(const Fe<NL>& lo, const Fe<NL>& hi, const Fe<NL>& r) {
  return fe_add<NL>(lo, fe_mul<NL>(fe_sub<NL>(hi, lo), r));
}
// the places of pair i of a table of 2 h elements
template <int ORDER> LCPC_DEV u64 at_lo(u64 i, u64) { return ORDER == SUMCHECK_LOW_FIRST ? 2 * i : i; }
template <int ORDER> LCPC_DEV u64 at_hi(u64 i, u64 h) { return ORDER == SUMCHECK_LOW_FIRST ? 2 * i + 1 : i + h; }

template <int NL, int ORDER, bool FUSED>
__global__ void __launch_bounds__(SUMCHECK_LANES) sumcheck_round_kernel(const RoundArgs<NL> p) {
  __shared__ u32 red[SM_W * SM_T * SM_D1 * NL];
  const u64 h = p.pairs, step = (u64)gridDim.x * SUMCHECK_LANES;
  const u32 d = p.tm.d, n_terms = p.tm.n_terms;
  Fe<NL> acc[SM_T][SM_D1];
#pragma unroll
  for (int m = 0; m < SM_T; m++)
#pragma unroll
    for (int t = 0; t < SM_D1; t++) acc[m][t] = fe_zero<NL>();

  for (u64 i = (u64)blockIdx.x * SUMCHECK_LANES + threadIdx.x; i < h; i += step) {
    if constexpr (FUSED) {
      // the two pairs of the 4 h inputs whose results are pair i of the bound table of 2 h elements
      for (u32 j = 0; j < p.n_tables; j++) {
        const u32* src = p.tab[j];
        u32* dst = p.out[j];
        const u64 a0 = ORDER == SUMCHECK_LOW_FIRST ? 4 * i : i, a1 = ORDER == SUMCHECK_LOW_FIRST ? 4 * i + 1 : i + 2 * h;
        const u64 b0 = ORDER == SUMCHECK_LOW_FIRST ? 4 * i + 2 : i + h, b1 = ORDER == SUMCHECK_LOW_FIRST ? 4 * i + 3 : i + 3 * h;
        const Fe<NL> x0 = fe_load<NL>(src + a0 * NL), x1 = fe_load<NL>(src + a1 * NL);
        const Fe<NL> y0 = fe_load<NL>(src + b0 * NL), y1 = fe_load<NL>(src + b1 * NL);
        fe_store<NL>(dst + at_lo<ORDER>(i, h) * NL, fe_bind<NL>(x0, x1, p.r));
        fe_store<NL>(dst + at_hi<ORDER>(i, h) * NL, fe_bind<NL>(y0, y1, p.r));
      }
    }
    static_for([&](auto mc) {
      constexpr int m = mc;
      if (m < n_terms) {
        Fe<NL> prod[SM_D1];
        const u32 nf = p.tm.n_factors[m];
        for (u32 k = 0; k < nf; k++) {
          const u32 tb = p.tm.table[m][k];
          const u32* src = FUSED ? p.out[tb] : p.tab[tb];
          Fe<NL> v = fe_load<NL>(src + at_lo<ORDER>(i, h) * NL);
          const Fe<NL> diff = fe_sub<NL>(fe_load<NL>(src + at_hi<ORDER>(i, h) * NL), v);
          static_for([&](auto tc) {
            constexpr int t = tc;
            if (t <= d) {
              if constexpr (t > 0) v = fe_add<NL>(v, diff);
              if (k) prod[t] = fe_mul<NL>(prod[t], v);
              else prod[t] = v;
            }
          }, std::make_integer_sequence<int, SM_D1>{});
        }
        static_for([&](auto tc) {
          constexpr int t = tc;
          if (t <= d) acc[m][t] = fe_add<NL>(acc[m][t], prod[t]);
        }, std::make_integer_sequence<int, SM_D1>{});
      }
    }, std::make_integer_sequence<int, SM_T>{});
  }

  // lane l takes lane l + off: lane 0 of a wave ends with the sum of its 64 lanes
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  static_for([&](auto mc) {
    constexpr int m = mc;
    if (m < n_terms) {
      static_for([&](auto tc) {
        constexpr int t = tc;
        if (t <= d) {
          Fe<NL> s = acc[m][t];
#pragma unroll 1
          for (int off = 32; off >= 1; off >>= 1) s = fe_add<NL>(s, fe_shfl_down<NL>(s, off));
          if (lane == 0) lds_put<NL>(red, SM_W * SM_T * SM_D1, (wave * SM_T + m) * SM_D1 + t, s);
        }
      }, std::make_integer_sequence<int, SM_D1>{});
    }
  }, std::make_integer_sequence<int, SM_T>{});
  __syncthreads();
  auto wg_sum = [&](u32 m, u32 t) {
    Fe<NL> s = lds_get<NL>(red, SM_W * SM_T * SM_D1, m * SM_D1 + t);
    for (u32 w = 1; w < SM_W; w++) s = fe_add<NL>(s, lds_get<NL>(red, SM_W * SM_T * SM_D1, (w * SM_T + m) * SM_D1 + t));
    return s;
  };
  if (gridDim.x == 1) {
    // the only workgroup: evals[t] = sum_m c_m S[m][t]
    const u32 t = threadIdx.x;
    if (t <= d) {
      Fe<NL> e = fe_zero<NL>();
      for (u32 m = 0; m < n_terms; m++) e = fe_add<NL>(e, fe_mul<NL>(wg_sum(m, t), p.coeff[m]));
      fe_store<NL>(p.evals + (u64)t * NL, e);
    }
  } else {
    const u32 e = threadIdx.x, d1 = d + 1;
    if (e < n_terms * d1) fe_store<NL>(p.work + ((u64)blockIdx.x * n_terms * d1 + e) * NL, wg_sum(e / d1, e % d1));
  }
}

template <int NL> struct FinishArgs {
  const u32* work;
  u32* evals;
  u32 n_groups, n_terms, d;
  Fe<NL> coeff[SM_T];
};
// K18b: workgroup t: evals[t] = sum_m c_m sum_g work[(g n_terms + m)(d + 1) + t]
template <int NL> __global__ void __launch_bounds__(SUMCHECK_LANES) sumcheck_finish_kernel(const FinishArgs<NL> p) {
  __shared__ u32 red[SM_W * NL];
  const u32 t = blockIdx.x, d1 = p.d + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Fe<NL> e = fe_zero<NL>();
  for (u32 m = 0; m < p.n_terms; m++) {
    Fe<NL> s = fe_zero<NL>();
    for (u32 g = threadIdx.x; g < p.n_groups; g += SUMCHECK_LANES) s = fe_add<NL>(s, fe_load<NL>(p.work + (((u64)g * p.n_terms + m) * d1 + t) * NL));
#pragma unroll 1
    for (int off = 32; off >= 1; off >>= 1) s = fe_add<NL>(s, fe_shfl_down<NL>(s, off));
    __syncthreads();                     // (the waves' sums of the term before have been read)
    if (lane == 0) lds_put<NL>(red, SM_W, wave, s);
    __syncthreads();
    if (threadIdx.x == 0) {
      for (u32 w = 1; w < SM_W; w++) s = fe_add<NL>(s, lds_get<NL>(red, SM_W, w));
      e = fe_add<NL>(e, fe_mul<NL>(s, p.coeff[m]));
    }
  }
  if (threadIdx.x == 0) fe_store<NL>(p.evals + (u64)t * NL, e);
}

template <int NL> struct BindArgs {
  const u32* in[SUMCHECK_MAX_TABLES];
  u32* out[SUMCHECK_MAX_TABLES];
  u64 h;
  Fe<NL> r;
};
// K19: element i of table blockIdx.y
template <int NL, int ORDER> __global__ void __launch_bounds__(SUMCHECK_LANES) sumcheck_bind_kernel(const BindArgs<NL> p) {
  const u64 i = (u64)blockIdx.x * SUMCHECK_LANES + threadIdx.x;
  if (i >= p.h) return;
  const u32* src = p.in[blockIdx.y];
  const Fe<NL> lo = fe_load<NL>(src + at_lo<ORDER>(i, p.h) * NL), hi = fe_load<NL>(src + at_hi<ORDER>(i, p.h) * NL);
  fe_store<NL>(p.out[blockIdx.y] + i * NL, fe_bind<NL>(lo, hi, p.r));
}

template <int NL, bool FUSED>
hipError_t round_launch(const SumcheckJob& j, const uint32_t* coeffs, const uint32_t* one, const uint32_t* r, uint32_t* evals, uint32_t* work,
                        hipStream_t st, uint32_t* n_launches) {
  RoundArgs<NL> p = {};
  FinishArgs<NL> q = {};
  for (uint32_t t = 0; t < j.n_tables; t++) {
    p.tab[t] = j.in[t];
    if (FUSED) p.out[t] = j.out[t];
  }
  p.n_tables = j.n_tables;
  p.tm.n_terms = j.n_terms;
  p.tm.d = sumcheck_degree(j.n_tables, j.terms, j.n_terms);
  for (uint32_t m = 0; m < j.n_terms; m++) {
    p.tm.n_factors[m] = j.terms[m].n_factors;
    for (uint32_t k = 0; k < j.terms[m].n_factors; k++) p.tm.table[m][k] = j.terms[m].table[k];
    p.coeff[m] = q.coeff[m] = fe_arg<NL>(coeffs ? coeffs + (size_t)m * NL : one);
  }
  p.pairs = sumcheck_pairs(j);
  if (FUSED) p.r = fe_arg<NL>(r);
  p.work = work; p.evals = evals;
  const uint32_t groups = sumcheck_groups(p.pairs, j.max_groups);
  if (j.order == SUMCHECK_LOW_FIRST) hipLaunchKernelGGL((sumcheck_round_kernel<NL, SUMCHECK_LOW_FIRST, FUSED>), dim3(groups), dim3(SUMCHECK_LANES), 0, st, p);
  else hipLaunchKernelGGL((sumcheck_round_kernel<NL, SUMCHECK_HIGH_FIRST, FUSED>), dim3(groups), dim3(SUMCHECK_LANES), 0, st, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (n_launches) *n_launches += 1;
  if (groups == 1) return hipSuccess;
  q.work = work; q.evals = evals; q.n_groups = groups; q.n_terms = j.n_terms; q.d = p.tm.d;
  hipLaunchKernelGGL((sumcheck_finish_kernel<NL>), dim3(q.d + 1), dim3(SUMCHECK_LANES), 0, st, q);
  e = hipGetLastError();
  if (e == hipSuccess && n_launches) *n_launches += 1;
  return e;
}

}  // namespace

hipError_t launch_sumcheck_bind(int nl, int order, const uint32_t* const* in, uint32_t* const* out, uint32_t n_tables, uint64_t n,
                                const uint32_t* r, hipStream_t st) {
  const SumcheckJob j = {nl, order, true, false, in, out, n_tables, nullptr, 0, n, nullptr, nullptr, 0, 0};
  if (!r || !sumcheck_job_ok(j)) return hipErrorInvalidValue;
  return with_nl(nl, [&](auto nlc) {
    constexpr int NL = nlc;
    BindArgs<NL> p = {};
    for (uint32_t t = 0; t < n_tables; t++) { p.in[t] = in[t]; p.out[t] = out[t]; }
    p.h = n / 2;
    p.r = fe_arg<NL>(r);
    const dim3 grid((unsigned)((p.h + SUMCHECK_LANES - 1) / SUMCHECK_LANES), n_tables);      // (h < 2^38: below 2^30 workgroups)
    if (order == SUMCHECK_LOW_FIRST) hipLaunchKernelGGL((sumcheck_bind_kernel<NL, SUMCHECK_LOW_FIRST>), grid, dim3(SUMCHECK_LANES), 0, st, p);
    else hipLaunchKernelGGL((sumcheck_bind_kernel<NL, SUMCHECK_HIGH_FIRST>), grid, dim3(SUMCHECK_LANES), 0, st, p);
    return hipGetLastError();
  });
}

hipError_t launch_sumcheck_round(int nl, int order, const uint32_t* const* tables, uint32_t n_tables, const SumcheckTerm* terms, uint32_t n_terms,
                                 const uint32_t* coeffs, const uint32_t* one, uint64_t n, uint32_t* evals, uint32_t* work, uint64_t work_elems,
                                 uint32_t max_groups, hipStream_t st, uint32_t* n_launches) {
  const SumcheckJob j = {nl, order, false, true, tables, nullptr, n_tables, terms, n_terms, n, evals, work, work_elems, max_groups};
  if (!one || !sumcheck_job_ok(j)) return hipErrorInvalidValue;
  if (n_launches) *n_launches = 0;
  return with_nl(nl, [&](auto nlc) {
    constexpr int NL = nlc;
    return round_launch<NL, false>(j, coeffs, one, nullptr, evals, work, st, n_launches);
  });
}

hipError_t launch_sumcheck_bind_round(int nl, int order, const uint32_t* const* in, uint32_t* const* out, uint32_t n_tables,
                                      const SumcheckTerm* terms, uint32_t n_terms, const uint32_t* coeffs, const uint32_t* one, uint64_t n,
                                      const uint32_t* r, uint32_t* evals, uint32_t* work, uint64_t work_elems, uint32_t max_groups,
                                      hipStream_t st, uint32_t* n_launches) {
  const SumcheckJob j = {nl, order, true, true, in, out, n_tables, terms, n_terms, n, evals, work, work_elems, max_groups};
  if (!one || !r || !sumcheck_job_ok(j)) return hipErrorInvalidValue;
  if (n_launches) *n_launches = 0;
  return with_nl(nl, [&](auto nlc) {
    constexpr int NL = nlc;
    return round_launch<NL, true>(j, coeffs, one, r, evals, work, st, n_launches);
  });
}

}  // namespace lcpc
