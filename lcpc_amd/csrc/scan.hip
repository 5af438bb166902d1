// lcpc_amd/csrc/scan.hip -- K17: prefix sums and prefix products of element vectors (include/lcpc_hip_scan.h), the one step of the
// univariate prover's chain whose elements depend on each other.
//
// THREE PHASES, AND NO SINGLE-PASS FORM.  A scan over more than one workgroup's tile needs every tile to learn the combination of all
// tiles before it.  Here kernel boundaries are the ONLY ordering between workgroups:
//   K17a  every workgroup reduces its tile of SCAN_LANES * SC_C consecutive elements of vector blockIdx.y to one element of `work`;
//   K17b  the tile totals of every vector are scanned in place (exclusive, seeded with c_v), which also gives total[v] -- by the same
//         three phases one level down, a recursion that ends where a vector's totals fit one tile: one launch of K17c for up to
//         scan_tile^2 elements per vector, three for up to scan_tile^3 (which is beyond the 2^39 elements a call takes);
//   K17c  every workgroup loads its tile again, scans it, combines with its prefix from `work` and stores.
// The single-pass alternatives (decoupled look-back, a flag in memory that a workgroup spins on, a cooperative grid sync, persistent
// workgroups) save the second read of the input, but in every one of them a workgroup WAITS for another, and a workgroup that waits
// for one that is not resident never ends: on a device shared with other work that is a hang of the whole device, not a slow call.
// They are ruled out on purpose.  Do not "optimise" this file into one of them; the price of the three-phase form is one more read
// of the input (two reads and one write against a map's two reads and one write) and is stated in DESIGN section 4.
//
// THE TILE.  The layout is blocked: lane l of a workgroup holds the SC_C CONSECUTIVE elements base + l SC_C + j, for sums and
// products alike (one body; a sum is bound by memory either way).  A tile is scanned in three steps:
//   1. the lane combines its elements into running values in registers (SC_C - 1 operations);
//   2. the lane totals are scanned across the wave by six shuffle steps, the wave totals go through LDS, and every lane combines the
//      totals of the waves before its own with the tile's seed (6 + SCAN_LANES / 64 operations per LANE);
//   3. every element is combined with the lane's exclusive prefix and stored (SC_C operations).
// All loads of a tile come before the barrier of step 2 and all its stores after it, and a workgroup reads and writes its own tile
// only: out == in is safe in both modes.  Per element that is (2 SC_C + 10) / SC_C operations in K17c (SC_C - 1, six for the wave
// scan, four for the wave totals, one for the lane's prefix, SC_C) and (SC_C + 5) / SC_C in K17a (six butterfly steps for the wave's
// reduction): 4.875 multiplies per element of a product at SC_C = 8 and 3.94 at 16, against the six per element that a striped layout
// (one wave scan per element) pays in K17c alone.  A lane's elements are SC_C * NL * 4 contiguous bytes (192 / 256 for Ft191 / Ft255
// at SC_C = 8, 128 / 256 for Ft63 / Ft127 at 16): every cache line a wave touches is used whole, but one load instruction of a wave
// spans 64 of them -- no access is coalesced per instruction.  Loading striped and transposing through LDS into the blocked layout
// is the alternative; it was not built and the two have not been measured against each other.
// SC_C is set by the registers the running values take, SC_C * NL: 64 for Ft255 and Ft127, 48 for Ft191, 32 for Ft63 (DESIGN section 4
// has the VGPR counts and the resident workgroups; no instantiation uses scratch).  Positions past the end of a vector act as the
// identity and store nothing.  K17b runs the same kernels on the totals, so scan_mid_chunk is scan_tile.
#include <utility>

#include "fft_dev.h"

namespace lcpc {

namespace {

// f(0), f(1), ... with the index a compile-time constant (quot.hip says why the loops are not left to the unroller)
template <class F, int... J> LCPC_DEV void static_for(F&& f, std::integer_sequence<int, J...>) { (f(std::integral_constant<int, J>{}), ...); }

template <int NL> constexpr int SC_C = (int)scan_lane_elems(NL);
constexpr u32 SC_W = SCAN_LANES / 64;

template <int NL> LCPC_DEV Fe<NL> fe_pick(bool c, const Fe<NL>& a, const Fe<NL>& b) {
  Fe<NL> r;
#pragma unroll
  for (int l = 0; l < NL; l++) r.v[l] = c ? a.v[l] : b.v[l];
  return r;
}
template <int NL, int OP> LCPC_DEV Fe<NL> sc_op(const Fe<NL>& a, const Fe<NL>& b) {
  if constexpr (OP == SCAN_SUM) return fe_add<NL>(a, b);
  else return fe_mul<NL>(a, b);
}
template <int NL> LCPC_DEV Fe<NL> fe_shfl_up(const Fe<NL>& a, u32 d) {
  Fe<NL> r;
#pragma unroll
  for (int l = 0; l < NL; l++) r.v[l] = __shfl_up(a.v[l], d, 64);
  return r;
}
template <int NL> LCPC_DEV Fe<NL> fe_shfl_xor(const Fe<NL>& a, int d) {
  Fe<NL> r;
#pragma unroll
  for (int l = 0; l < NL; l++) r.v[l] = __shfl_xor(a.v[l], d, 64);
  return r;
}

// The tile of one workgroup of SCAN_LANES lanes.  load(j): the lane's j-th element (the identity for a position past the end);
// store(j, r): r = seed (+) every element of the tile up to and including that one (inclusive) or before it (exclusive).  Returns
// seed (+) the whole tile, in every lane.  lds: SC_W * NL words; the caller puts a barrier before the next use of them
template <int NL, int OP, class Load, class Store>
LCPC_DEV Fe<NL> tile_scan(u32* lds, const Fe<NL>& ident, const Fe<NL>& seed, bool exclusive, Load load, Store store) {
  constexpr int C = SC_C<NL>;
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Fe<NL> pre[C];
  static_for([&](auto jc) {
    constexpr int j = jc;
    const Fe<NL> x = load(j);
    if constexpr (j > 0) pre[j] = sc_op<NL, OP>(pre[j - 1], x);
    else pre[j] = x;
  }, std::make_integer_sequence<int, C>{});
  Fe<NL> inc = pre[C - 1];
  static_for([&](auto kc) {
    constexpr u32 d = 1u << kc;
    const Fe<NL> r = sc_op<NL, OP>(fe_shfl_up<NL>(inc, d), inc);
    inc = fe_pick<NL>(lane >= d, r, inc);
  }, std::make_integer_sequence<int, 6>{});
  if (lane == 63) lds_put<NL>(lds, SC_W, wave, inc);
  Fe<NL> ex = fe_pick<NL>(lane != 0, fe_shfl_up<NL>(inc, 1), ident);
  __syncthreads();
  Fe<NL> run = seed, before = seed;
#pragma unroll
  for (u32 k = 0; k < SC_W; k++) {
    before = fe_pick<NL>(k == wave, run, before);
    run = sc_op<NL, OP>(run, lds_get<NL>(lds, SC_W, k));
  }
  ex = sc_op<NL, OP>(before, ex);
  static_for([&](auto jc) {
    constexpr int j = jc;
    Fe<NL> own = pre[j];
    if constexpr (j > 0) own = fe_pick<NL>(exclusive, pre[j - 1], own);
    else own = fe_pick<NL>(exclusive, ident, own);
    store(j, sc_op<NL, OP>(ex, own));
  }, std::make_integer_sequence<int, C>{});
  return run;
}

// K17a: work[v * tiles + t] = the combination of tile t of vector v
template <int NL, int OP> __global__ void __launch_bounds__(SCAN_LANES) scan_reduce_kernel(const u32* in, u32* work, u64 n, Fe<NL> ident) {
  __shared__ u32 lds[SC_W * NL];
  constexpr int C = SC_C<NL>;
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 base = (u64)blockIdx.x * scan_tile(NL) + (u64)threadIdx.x * C;
  const u32* src = in + (u64)blockIdx.y * n * NL;
  Fe<NL> acc = ident;
  static_for([&](auto jc) {
    constexpr int j = jc;
    const u64 i = base + j;
    const Fe<NL> x = i < n ? fe_load<NL>(src + i * NL) : ident;
    if constexpr (j > 0) acc = sc_op<NL, OP>(acc, x);
    else acc = x;
  }, std::make_integer_sequence<int, C>{});
  static_for([&](auto kc) {
    constexpr int d = 32 >> kc;
    acc = sc_op<NL, OP>(acc, fe_shfl_xor<NL>(acc, d));
  }, std::make_integer_sequence<int, 6>{});
  if (lane == 0) lds_put<NL>(lds, SC_W, wave, acc);
  __syncthreads();
  if (threadIdx.x == 0) {
    Fe<NL> r = lds_get<NL>(lds, SC_W, 0);
#pragma unroll
    for (u32 k = 1; k < SC_W; k++) r = sc_op<NL, OP>(r, lds_get<NL>(lds, SC_W, k));
    fe_store<NL>(work + ((u64)blockIdx.y * gridDim.x + blockIdx.x) * NL, r);
  }
}

template <int NL> struct ScanArgs {
  const u32* in;
  u32* out;
  const u32* seeds;    // element v * gridDim.x + t seeds tile t of vector v (K17b's prefixes; init for one tile); null: the identity
  u32* total;          // one tile only: total[v]; null otherwise
  u64 n;
  u32 exclusive;
  Fe<NL> ident;
};

// K17c: tile blockIdx.x of vector blockIdx.y
template <int NL, int OP> __global__ void __launch_bounds__(SCAN_LANES) scan_apply_kernel(ScanArgs<NL> p) {
  __shared__ u32 lds[SC_W * NL];
  constexpr int C = SC_C<NL>;
  const u64 base = (u64)blockIdx.x * scan_tile(NL) + (u64)threadIdx.x * C;
  const u32* src = p.in + (u64)blockIdx.y * p.n * NL;
  u32* dst = p.out + (u64)blockIdx.y * p.n * NL;
  const Fe<NL> seed = p.seeds ? fe_load<NL>(p.seeds + ((u64)blockIdx.y * gridDim.x + blockIdx.x) * NL) : p.ident;
  const Fe<NL> all = tile_scan<NL, OP>(
      lds, p.ident, seed, p.exclusive != 0,
      [&](int j) { return base + j < p.n ? fe_load<NL>(src + (base + j) * NL) : p.ident; },
      [&](int j, const Fe<NL>& r) {
        if (base + j < p.n) fe_store<NL>(dst + (base + j) * NL, r);
      });
  if (p.total && threadIdx.x == 0) fe_store<NL>(p.total + (u64)blockIdx.y * NL, all);
}

inline bool meet(const uint32_t* a, uint64_t na, const uint32_t* b, uint64_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return a && b && x < y + nb * 4 && y < x + na * 4;
}

// one level: the scan of n_vecs runs of n elements, and below it the scan of their tile totals in place in `work`
template <int NL, int OP>
hipError_t scan_launch(int mode, const uint32_t* in, uint32_t* out, uint64_t n, uint32_t n_vecs, const uint32_t* init, uint32_t* total,
                       const Fe<NL>& ident, uint32_t* work, hipStream_t st, uint32_t* n_launches) {
  const uint64_t tiles = scan_tiles(NL, n);                                       // (below SCAN_MAX_TILES)
  ScanArgs<NL> p;
  p.in = in; p.out = out; p.n = n; p.exclusive = mode == SCAN_EXCLUSIVE; p.ident = ident;
  const dim3 grid((unsigned)tiles, n_vecs), lanes(SCAN_LANES);
  if (tiles == 1) {
    p.seeds = init; p.total = total;
    hipLaunchKernelGGL((scan_apply_kernel<NL, OP>), grid, lanes, 0, st, p);
    if (n_launches) *n_launches += 1;
    return hipGetLastError();
  }
  hipLaunchKernelGGL((scan_reduce_kernel<NL, OP>), grid, lanes, 0, st, in, work, (u64)n, ident);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (n_launches) *n_launches += 1;
  // K17b: the totals become the tiles' prefixes, by the same scan one level down, behind this level's totals in `work`
  e = scan_launch<NL, OP>(SCAN_EXCLUSIVE, work, work, tiles, n_vecs, init, total, ident, work + tiles * n_vecs * NL, st, n_launches);
  if (e != hipSuccess) return e;
  p.seeds = work; p.total = nullptr;
  hipLaunchKernelGGL((scan_apply_kernel<NL, OP>), grid, lanes, 0, st, p);
  if (n_launches) *n_launches += 1;
  return hipGetLastError();
}

}  // namespace

hipError_t launch_scan(int nl, int op, int mode, const uint32_t* in, uint32_t* out, uint64_t n, uint32_t n_vecs, const uint32_t* init,
                       uint32_t* total, const uint32_t* one, uint32_t* work, uint64_t work_elems, hipStream_t st, uint32_t* n_launches) {
  if (!nl_ok(nl) || (op != SCAN_SUM && op != SCAN_PRODUCT) || (mode != SCAN_INCLUSIVE && mode != SCAN_EXCLUSIVE) || !in || !out || !one || !work) return hipErrorInvalidValue;
  if (n == 0 || n >= ((uint64_t)1 << 39) || n_vecs == 0 || n_vecs > 65535 || n * n_vecs >= ((uint64_t)1 << 39)) return hipErrorInvalidValue;   // (no overflow: 2^55)
  if (scan_tiles(nl, n) >= SCAN_MAX_TILES) return hipErrorInvalidValue;                                  // (the grid: tiles * 256 lanes < 2^32)
  if (!elem_aligned(in, nl) || !elem_aligned(out, nl) || !elem_aligned(work, nl) || work_elems < scan_work_elems(nl, n, n_vecs)) return hipErrorInvalidValue;
  if ((init && !elem_aligned(init, nl)) || (total && !elem_aligned(total, nl))) return hipErrorInvalidValue;
  const uint64_t words = n * n_vecs * nl, ends = (uint64_t)n_vecs * nl, ww = scan_work_elems(nl, n, n_vecs) * nl;
  if (in != out && meet(in, words, out, words)) return hipErrorInvalidValue;
  for (const uint32_t* data : {in, (const uint32_t*)out})
    if (meet(init, ends, data, words) || meet(total, ends, data, words) || meet(work, ww, data, words)) return hipErrorInvalidValue;
  if (meet(init, ends, total, ends) || meet(work, ww, init, ends) || meet(work, ww, total, ends)) return hipErrorInvalidValue;
  if (n_launches) *n_launches = 0;
  return with_nl(nl, [&](auto nlc) {
    constexpr int NL = nlc;
    if (op == SCAN_SUM) return scan_launch<NL, SCAN_SUM>(mode, in, out, n, n_vecs, init, total, fe_arg<NL>(nullptr), work, st, n_launches);
    return scan_launch<NL, SCAN_PRODUCT>(mode, in, out, n, n_vecs, init, total, fe_arg<NL>(one), work, st, n_launches);
  });
}

}  // namespace lcpc
