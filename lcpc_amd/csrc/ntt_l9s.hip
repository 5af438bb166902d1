// lcpc_amd/csrc/ntt_l9s.hip -- K1s: the shape-specialised Ft255 row NTT (LcEncoding::encode for Ligero,
// lcpc-ligero-pc/src/lib.rs:162-164 = fffft fft_io_pc [3P]) for the two-pass plans on 1024-element tiles
// (2^11 <= n_cols <= 2^20, which covers BASELINE.json's Ligero configs) and, built from the same two kernels, three-pass plans
// for 2^21 .. 2^26 columns (kernels.h ntt_l9s3_supported).
//
// Same tiling, same lazy signed 9 x 29-bit arithmetic and the same canonical-output trick as ntt_pass_l9_kernel
// (kernels.hip, which stays the general kernel: one pass, three passes, 2048-element tiles); what differs is where the
// non-multiplier instructions went (profiles/r02_ntt_lab_*.txt: the kernel is VALU-issue bound, every instruction counts):
//   * the pass shape -- S stages on 2^S x 2^LTJ tiles, first or last pass -- is a template parameter, so the index
//     math of a round is a handful of shifts instead of ~40 instructions on run-time shifts and masks;
//   * twiddles come from a per-pass PACK in lane order: for tile class c (first pass: the tile's position in the row;
//     last pass: one class) and round r the twiddles of quad q sit at [c][r][variant][chunk][q mod period], so a wave
//     reads 1 KiB runs instead of gathering 64 x 48-byte table entries at strides of up to 12 KiB;
//   * normalise + clamp of the pure-sum output are one carry pass (ln::clamp_apply), done before the multiplier
//     chains start so that the sum does not occupy registers across them (no scratch spills at 128 VGPRs);
//   * the first pass stores values in [0, p + 2^239) (< 2^256, what its successor reads as limbs anyway) without the
//     final conditional subtract; the last pass does that subtract only for the rare waves that need it;
//   * an odd stage count is peeled as a radix-2 round at stage 0, where a zero-padded row (rate <= 1/2) needs no
//     additions at all: (x, 0) -> (x, x w).
//   * (round 6) a tile makes no LDS round trip it does not need: the four elements a thread loads are its first round's quad, which
//     therefore runs from the registers with no barrier before it; the last pass's final round owns four consecutive elements and
//     reduces and stores them itself;
//   * the pure first pass's final round (I only) does the same for the packed intermediate: its quad is four elements of one column,
//     clamped, packed and stored from the registers; and every round that stores from registers clamps each output once, straight
//     from the butterfly's sums (ntt_ln_dev.h clamp_store; the bounds: field_ln.h clamp_apply);
//   * (round 6) a wave holds priority 1 while it issues memory instructions and 0 inside the multiplier chains (field_dev.h mem_phase);
//   * every global address is a wave-uniform 64-bit base in scalar registers plus an unsigned 32-bit byte offset per lane (the kernel's
//     "Global addresses"; ntt_ln_dev.h ubase / lane_at / pack_get_u): no 64-bit vector shifts or carry adds for addresses.
// Exact modular arithmetic: any stage grouping gives the same fully-reduced bits as the reference's radix-2 loop.
#include "kernels.h"
#include "ntt_ln_dev.h"

namespace lcpc {

namespace {

// twiddle pack of one (class, round) (layout: ntt_ln_dev.h pack_get; built by ntt_lns.hip): radix-4 rounds: variants 0 w0, 1 w3,
// 2 w2 (plain table, w^i * 2^261) and 3, 4, 5 the same from the converting table (w^i * 2^5); the radix-2 round: 0 w, 1 converting w.
//
// The radix-4 butterfly of stages (t, t + 1) on x0 .. x3 (quarter-block apart), radix-2 DIF regrouped:
//   b0 = x0 + x2, b1 = x1 + x3, b2 = (x0 - x2) w0, b3 = (x1 - x3) w1;  c0 = b0 + b1, c1 = (b0 - b1) w2, c2 = b2 + b3, c3 = (b2 - b3) w2
// with w0 = w^e, w1 = w^(e + n/4) = I w0 (I = w^(n/4), the field's fixed primitive 4th root of unity) and w2 = w0^2.  Hence
//   t = (x1 - x3) I;  c2 = ((x0 - x2) + t) w0;  c3 = ((x0 - x2) - t) w3,  w3 = w0 w2 = w^(3 e):
// I is ONE constant for every lane of every transform, so its multiply takes the shifted-multiples form with scalar operands
// (ln::mul_u on a.wq_w: 119 instructions; the code calls ln::mul_us, the same multiply with the two-instruction tail: two fewer) and a generic round does three lane-varying Montgomery multiplies (188 each) instead
// of four; c2 comes out of a multiplier normalised.  Exact arithmetic mod p: the same fully reduced bits.
// MID: the intermediate between the two passes is not the packed comm buffer but a.mid, which holds every element as the
// LDS tile holds it -- 9 signed 29-bit limbs, normalised; DIF form: |value| < 4p (invariant I of field_ln.h); pure form: |value| <
// 12.04p, the I-only round's c1, c2, c3 as they leave the butterfly (below: the coset pass's round 0 is built for that) -- laid out per
// row as the successor's tiles: [tile of 1024 elements][limbs 0-3 x 1024 | limbs 4-7 x 1024 | limb 8 x 1024] (36 KiB per tile).
// The first pass then stores its tile as it stands (no clamp, no reduction, no 29 -> 32-bit packing: ~60 VALU per element)
// and the last pass's tile load is a plain 36 KiB copy into LDS (no unpacking: ~17 per element), at 36 instead of 32 bytes
// per element of intermediate traffic on a kernel that HBM does not bind.
//
// NF, the pure / coset form of the two-pass plans (a.form).  With a column index n = b + 1024 i and a frequency
// k = k1 + 2^S k2 (S = log n - 10 first-pass stages),
//   X[k] = sum_b w^(b k1) w1024^(b k2) ( sum_i x[b + 1024 i] w_{2^S}^(i k1) ):
// the inner sum is a plain 2^S-point DFT whose twiddles do not depend on b, and the "twist" w^(b k1) can ride on the stage twiddles of
// either pass.  The DIF form above lets the first pass carry it; here the last pass does:
//   * first pass, pure: a 2^S-point DIF per column, one pack class for every tile, row and lp.  Distinct twiddle triples per radix-4
//     round: 4^(NR4 - 1), .., 16, 4, 1 (ntt_ln_dev.h PureShape) -- the round with 4 is wave-uniform (waves dealt by j mod 4), the round
//     with 1 multiplies by I only;
//   * last pass, coset: tile t (it holds k1 = rev_S(t) of every column) evaluates its 1024 coefficients on g_t <w1024>, g_t = w^k1, by
//     multiply-then-butterfly rounds over z^m - gamma (natural order in, bit-reversed out): in round r = 0 .. 4 the quad x0 .. x3
//     (a quarter of its sub-block apart) of sub-block m < 4^r takes the triple w, w^2, w^3 with w = W^E,
//     E = 2^(8 - 2r) (k1 + 2^S rev_2r(m)) < n / 4:
//       p_i = x_i w^i;  t = (p1 - p3) I;  y0 = (x0 + p2) + (p1 + p3), y1 = (x0 + p2) - (p1 + p3), y2 = (x0 - p2) + t, y3 = (x0 - p2) - t.
//     Round 0's triple is one per tile and round 1's one per wave (wave = sub-block, no special deal of the lanes): ln::mul_u; rounds
//     2, 3, 4 have 16, 64, 256 triples: ln::mul from the pack, which is per tile class and read in the XCD-aware order that keeps the
//     rows of one tile position back to back.
// Per quad chain of the headline (8 + 10): 6 + 9 lane-varying and 7 + 11 uniform multiplies against 9 + 9 and 7 + 8.
// Canonical output: block 0 of the pure pass is the low sub-block of EVERY tile; it leaves through the converting twiddles as before,
// and the pure sum that would carry it on is converted in round RC (PureShape), so the coset pass sees canonical values only.
// M2, the multiplier of the lane-varying rounds of the pure / coset form (NttPackInfo.mul2; the plan chooses it per pass, ctx.cpp
// build_limb_plan): ln::mul on one pack entry w c 2^261 (188 instructions), or ln::mul2 on the pair b0 = w c 2^145, b1 = w c 2^290 that a
// split pack holds for every lane-varying slot (148).  Where the bounds below name the output of ln::mul, (-1.2p, 0.2p], mul2 returns
// (-3.01p, 2.01p) for limbs in (-2^30, 2^30) -- still |value| < 4p, invariant I; the rounds that depend on more say so.
template <bool M2> struct Tw { LN<9> b0, b1; };
template <> struct Tw<false> { LN<9> b0; };
// variant uv + lv: uv wave-uniform, lv by lane (ntt_ln_dev.h pack_get_u: scalar bases, 32-bit lane offsets)
template <bool M2, u32 NV> LCPC_DEV Tw<M2> tw_get(const u32* blk, u32 period, u32 uv, u32 lv, u32 jl) {
  Tw<M2> t;
  if constexpr (M2) {
    t.b0 = pack_get_u<2 * NV>(blk, period, uv, lv, jl);
    t.b1 = pack_get_u<2 * NV>(blk, period, NV + uv, lv, jl);
  } else {
    t.b0 = pack_get_u<NV>(blk, period, uv, lv, jl);
  }
  return t;
}
template <bool M2> LCPC_DEV LN<9> tw_mul(const LN<9>& x, const Tw<M2>& w) {
  if constexpr (M2) return ln::mul2<LnField<FT255>>(x, w.b0, w.b1);
  else return ln::mul<LnField<FT255>>(x, w.b0);
}

template <int S, int LTJ, bool FIRST, bool MID, bool NF, bool M2>
__global__ void __launch_bounds__(256, 4) ntt_pass_l9s_kernel(NttPassArgs a, const u32* __restrict__ pack, NttPackInfo pi) {
  using FT = LnField<FT255>;
  constexpr int NL = 8, LT = S + LTJ, LBT = LTJ;
  constexpr bool LAST = !FIRST;
  static_assert(LT == 10, "1024-element tiles: one radix-4 quad (two radix-2 pairs) per thread and round");
  static_assert(FIRST || (LTJ == 0 && S % 2 == 0), "the last pass works on contiguous tiles and ends with the trivial stages k-2, k-1");
  static_assert(NF || !M2, "the two-table multiply serves the pure / coset form only");
  using SH = Shape<S, LBT>;
  using SP = PureShape<S>;
  constexpr int RU = NF ? (FIRST ? SP::RU : -1) : SH::RU;   // (the coset pass's two uniform rounds need no deal of the lanes)
  constexpr int RC = NF && FIRST ? SP::RC : -1;
  // a pass with a uniform round reads its tile with a lane stride of 16 elements there (64-way bank conflicts on the uint4
  // planes): the tile is kept XOR-swizzled -- element e at slot e ^ ((e >> 4) & 15), a permutation inside every aligned block
  // of 16 -- which leaves the consecutive accesses of the other rounds conflict-free and spreads that round's over all banks.
  // The new form keeps a swizzle, chosen from the bank arithmetic of a 16-lane group (16 uint4 slots = one 256-byte bank row):
  //   * coset pass: no uniform deal, but round 3 reads lanes (m, q & 3) at element 16 m + (q & 3) + 4 k and round 4 lane q at 4 q + k
  //     (k = 0 .. 3 the quad's four reads): without a swizzle a group meets 4 of the 16 slots.  With b = bits 4-5 of the element
  //     XORed into BOTH bit pairs of the slot (e ^ 5 b), round 3's group maps (q & 3, m & 3) -> ((q & 3) ^ m, k ^ m) and round 4's
  //     (q & 3, (q >> 2) & 3) -> (k ^ b, (q & 3) ^ b): 16 distinct slots each; rounds 0 .. 2 read runs of >= 16 consecutive elements, which
  //     any permutation inside the aligned blocks of 16 leaves conflict-free;
  //   * pure pass at the headline's LBT = 2: the uniform round's lanes (m, lp) read element 64 m + 4 w + lp + 16 k and the I-only
  //     round's lanes (j, lp) read 16 j + lp + 4 k: bits 4-5 XOR bits 6-7 of the element, XORed into slot bits 2-3, give the group
  //     (lp, w ^ m ^ k) and (lp, k ^ j) -- 16 distinct slots each.  Other first passes with a uniform round keep the DIF form's swizzle
  //     (LBT = 0: lanes 16 and 4 elements apart, which it was made for).
  constexpr bool SWZD = NF ? (LAST || SP::RU >= 0) : RU >= 0;
  auto SWZ = [](u32 e) -> u32 {
    if constexpr (NF && LAST) return e ^ (((e >> 4) & 3u) * 5u);
    else if constexpr (NF && FIRST && SWZD && LBT == 2) return e ^ ((((e >> 4) ^ (e >> 6)) & 3u) << 2);
    else if constexpr (SWZD) return e ^ ((e >> 4) & 15u);
    else return e;
  };
  extern __shared__ __attribute__((aligned(16))) u32 lds[];
  constexpr u32 T = 1u << LT;
  u32* nqp = lds + (size_t)T * 9;                            // NEGATED q*p rows (ln::clamp_apply)
  const u32 k = a.log_n;
  const u32 tiles_per_row = 1u << (k - LT);
  u64 row;
  u32 tile;
  if (FIRST && a.tile_group) {
    // short runs: 2^tile_group neighbouring tiles touch the same 128-byte lines / DRAM pages.  They go to one XCD (workgroups
    // are dealt to the XCDs round-robin) as consecutive workgroups, so that a line one of them fetched is in that L2 when the
    // others ask for it and their partial-line stores meet there before the write-back (host: ntt_tile_group, ctx.cpp)
    const u32 lg = a.tile_group;
    const u32 xcd = blockIdx.x & 7u;
    const u64 qq = blockIdx.x >> 3;
    const u32 sub = (u32)qq & ((1u << lg) - 1);
    const u64 q2 = qq >> lg;
    tile = (((u32)(q2 / a.n_rows) * 8u + xcd) << lg) | sub;
    row = q2 % a.n_rows;
  } else if (tiles_per_row >= 8) {                           // XCD-aware order, as in ntt_pass_kernel
    const u32 xcd = blockIdx.x & 7u;
    const u64 qq = blockIdx.x >> 3;
    tile = (u32)(qq / a.n_rows) * 8u + xcd;
    row = qq % a.n_rows;
  } else {
    row = blockIdx.x / tiles_per_row;
    tile = blockIdx.x % tiles_per_row;
  }
  const u32 tid = threadIdx.x;
  mem_phase(true);                                           // (field_dev.h: wave priority while a wave issues its memory instructions)
  const u32 lb = FIRST ? k - S : 0u;                         // index bits below the pass's stage field
  // element index of LDS slot e = (i << LBT) | lp.  First pass: (i << lb) | (tile << LTJ) | lp; last pass: tile * 2^S + i
  auto gindex = [&](u32 e) -> u32 {
    if constexpr (FIRST) return ((e >> LBT) << lb) | (tile << LTJ) | (e & ((1u << LBT) - 1));
    else return (tile << S) | e;
  };
  const bool canon = a.roots29c != nullptr && ((u32)row & a.canon_row_mask) == 0;     // (wave-uniform)
  for (u32 i = tid; i < 64 * 12; i += 256) nqp[i] = 0u - *lane_at(ubase(a.qp29), i * 4u);
  // Global addresses (ntt_ln_dev.h ubase / lane_at): the row, the tile of a last pass and the pack class are the workgroup's own --
  // 64-bit, scalar -- and a lane adds an unsigned 32-bit byte offset.  The largest a lane forms: first pass, an element of its row,
  // gindex(e) * 32 < 2^k * 32 <= 2^31 (k <= 26, the three-pass plans; launch_ntt_pass_l9s refuses more); last pass, an element of its
  // tile, < 32 KiB (36 KiB in the limb intermediate); the limb intermediate's store, < 2^S tiles of 36 KiB <= 36 MiB.
  const u64 src_row = row * a.src_stride;                    // (flat element index of the row's start)
  const u32* src = ubase(a.src + (src_row + (FIRST ? 0u : (u64)tile << S)) * NL);
  const u32 n_val = (u32)(a.n_valid < ((u64)1 << k) ? a.n_valid : (u64)1 << k);      // (column indices are < 2^k: their comparisons stay 32-bit)
  constexpr bool DIRECT = !(LAST && MID);                    // the first round takes its inputs from the loads (below)
  LN<9> xin[4];
  if constexpr (LAST && MID) {
    // the tile as the first pass left it: [limbs 0-3][limbs 4-7][limb 8] planes, the LDS layout itself
    const uint4* t4 = reinterpret_cast<const uint4*>(ubase(a.mid + (row << k) * 9 + (size_t)tile * (9 * T)));   // (u32 indices below: < 36 KiB)
    uint4* l4 = reinterpret_cast<uint4*>(lds);
    if constexpr (SWZD) {
      // (the swizzled tile: planes 0 and 1 move whole uint4s, the limb-8 plane word by word -- (e + j) -> SWZ(e) ^ j for e = 0 mod 4)
#pragma unroll
      for (u32 i = tid; i < 2 * T; i += 256) l4[(i & ~(T - 1)) | SWZ(i & (T - 1))] = t4[i];
#pragma unroll
      for (u32 i = tid; i < T / 4; i += 256) {
        const uint4 v = t4[2 * T + i];
        const u32 b = 8 * T + SWZ(4 * i);
        lds[b] = v.x; lds[b ^ 1u] = v.y; lds[b ^ 2u] = v.z; lds[b ^ 3u] = v.w;
      }
    } else {
#pragma unroll
    for (u32 i = tid; i < 9 * T / 4; i += 256) l4[i] = t4[i];
    }
  } else {
    // The four elements a thread loads, e = tid + 256 it, ARE the quad (the two pairs) of its first round: dq = 256 there whatever the
    // pass shape.  They go to that round in registers -- no LDS round trip and, where that round needs no clamp table, no barrier
#pragma unroll
  for (u32 it = 0; it < 4; it++) {
    const u32 e = tid + 256u * it;
    Fe<NL> v;
    if constexpr (FIRST) {        // zero padding, the ragged tail of the caller's vector and the coeffs copy exist here only
      const u32 g = gindex(e);
      // (columns of this row that the caller's vector holds: n_valid, less where the flat vector ends inside the row or before it)
      const u64 left = a.n_src_total > src_row ? a.n_src_total - src_row : 0;
      const u32 n_src = left < n_val ? (u32)left : n_val;
      v = g < n_src ? fe_load<NL>(lane_at(src, g * (NL * 4u))) : fe_zero<NL>();
      if (a.copy_dst != nullptr && g < n_val) fe_store<NL>(lane_at(ubase(a.copy_dst + src_row * NL), g * (NL * 4u)), v);
    } else {
      v = fe_load<NL>(lane_at(ubase(src + 256u * it * NL), tid * (NL * 4u)));   // < 2^256 (the first pass's store), not necessarily < p
    }
    xin[it] = ln::from_packed<FT>(v);
  }
  __builtin_amdgcn_sched_barrier(0);                         // (the first round's twiddle loads stay behind the conversions: registers)
  }
  // (pack classes: DIF first pass and coset last pass one per tile position; DIF last pass and pure first pass one)
  const u32* cls_pack = ubase(pack + (size_t)(FIRST != NF ? tile : 0u) * pi.class_words);
  // tiles that hold elements of "block 0" (never multiplied so far).  a.blk0_gone: an earlier pass had a uniform round and
  // converted what was left of block 0 before it (below): nothing is in Montgomery form any more
  const bool blk0_tile = (FIRST || tile == 0) && a.blk0_gone == 0;   // (pure first pass: every tile holds its columns' block 0)
  LN<9> k32;                                                 // 2^5 = 2^261 R^-1: ln::mul by it converts (Montgomery form -> canonical)
#pragma unroll
  for (int i = 0; i < 9; i++) k32.v[i] = i == 0 ? 32u : 0u;
  const bool zero_hi = FIRST && n_val <= (1u << (k - 1));
  // the limb intermediate's tile sits in LDS; otherwise only the q*p table does, which no first round reads (their pure sums are
  // sums of loads: normalised, not clamped): the barrier at the end of that round serves
  if constexpr (!DIRECT) __syncthreads();

  if constexpr (SH::U0 == 1) {
    // ---- radix-2 round at stage 0 (odd S): pairs (e1, e1 + half), twiddle w^(index of e1).  Inputs straight from the
    //      loads (< p).  Stage 0 is all block 0: with canonical output the product takes the converting table.
    constexpr u32 half = 1u << (S - 1 + LBT);
    const u32* blk = cls_pack + pi.round_off[0];
#pragma unroll
    for (u32 pp = 0; pp < 2; pp++) {
      const u32 e1 = tid + 256u * pp;                        // slots with the top stage bit clear are [0, half)
      // pure form: w_{2^S}^i for the pair's i = e1 >> LBT, whatever the tile and lp
      const Tw<M2> w = NF ? tw_get<M2, 2>(blk, 1u << (S - 1), 0, canon ? 1u : 0u, e1 >> LBT) : tw_get<M2, 2>(blk, SH::period2, 0, canon ? 1u : 0u, e1);
      const LN<9> x = DIRECT ? xin[pp] : planes_get<FT>(lds, T, SWZ(e1));
      if (pp == 0) mem_phase(false);
      // pure form, S = 1 and 3: no later round reads the pack, so the sum half is converted here as well (RC < 0, ntt_ln_dev.h)
      const bool cvs = NF && canon && SH::NR4 <= 1;
      if (zero_hi) {
        if constexpr (DIRECT) planes_put<FT>(lds, T, SWZ(e1), cvs ? ln::mul<FT>(x, k32) : x);
        planes_put<FT>(lds, T, SWZ(e1 + half), tw_mul<M2>(x, w));           // (x, 0) -> (x, x w)
      } else {
        const LN<9> y = DIRECT ? xin[pp + 2] : planes_get<FT>(lds, T, SWZ(e1 + half));
        LN<9> sum = ln::add(x, y);                              // [0, 2p)
        ln::normalize<FT>(sum);
        planes_put<FT>(lds, T, SWZ(e1), cvs ? ln::mul<FT>(sum, k32) : sum);
        planes_put<FT>(lds, T, SWZ(e1 + half), tw_mul<M2>(ln::sub(x, y), w));
      }
    }
    mem_phase(true);
    __syncthreads();
  }

  const u32 q = tid;                                         // one quad per thread per radix-4 round (T / 4 == 256)
  if constexpr (NF && LAST) {
    // ---- the coset form (head comment): five multiply-then-butterfly rounds, thread q on quad q of its round throughout.
    //      What the tile holds between rounds is NOT invariant I: y1, y2, y3 are stored as they come out, un-normalised.  Per round:
    //      (M2: where two figures stand as a / b, a is ln::mul's and b ln::mul2's, whose products lie in (-3.01p, 2.01p).)
    //        x0            round 0: a load (< 2^256, or the limb intermediate: normalised, |value| < 10.8p / 12.04p -- the pure pass's
    //                      I-only round) ; later: limbs in (-2^30, 2^30), |value| < 12.1p.  Clamped first (but for the packed loads): [0, p + 2^239).
    //                      ln::clamp_apply's carry pass is signed, and its quotient estimate from the un-normalised top limb is off by
    //                      the carries still below it, here in [-2, 2] instead of [0, 3]: V - q p >= (QBIAS - |q| - 2.01) B > 0 and
    //                      < (PTOP + 1 + QBIAS + |q| + 3.01) B < p + 64 B for |q| <= 18, the margins field_ln.h states
    //        x1, x2, x3    rounds 0, 1 (ln::mul_u): normalised -- round 0's inputs are loads, and round 0 normalises all four outputs
    //                      for round 1 (mul_u wants sum |limb| < 9 * 2^29; top limb: |value| < 12.1p is < 2^27);
    //                      rounds 2 .. 4 (ln::mul / ln::mul2): limbs in (-2^30, 2^30), |value| < 9.1p < 16p (mul2 asks for the limbs only)
    //        p1, p2, p3    normalised; mul_u: (-2p, 2.7p), mul: (-1.2p, 0.2p], mul2: (-3.01p, 2.01p)
    //        t             mul_u of p1 - p3 (a difference of two normalised values): normalised, (-2p, 2.7p)
    //        y0            x0 + p2 + p1 + p3: limbs [0, 2^31 - 4] -- normalised before it is stored (the one output that needs headroom)
    //        y1            (x0 + p2) - (p1 + p3): limbs (-2^30, 2^30);  y2, y3 = (x0 - p2) +- t: limbs (-2^30, 2^30)
    //        |y|           round 0: < 4p + 3 * 2.7p = 12.1p (x0 un-clamped from the packed loads: < 2.5p + 8.1p); round 1: < 1.001p + 8.1p = 9.1p;
    //                      rounds 2 .. 4: < 1.001p + 3.6p = 4.6p; M2: y0 in (-9.03p, 7.04p), y1 in (-7.03p, 9.04p) (x0 + p2 in (-3.01p, 3.02p),
    //                      p1 + p3 in (-6.02p, 4.02p)), y2, y3 in (-4.71p, 6.72p) (x0 - p2 in (-2.01p, 4.02p), t in (-2p, 2.7p)): |y| < 9.04p,
    //                      inside the clamp's |q| <= 18 and mul_u's limb sums (p1 - p3: a difference of two normalised values)
    //      The final round reduces and stores its four consecutive elements from the registers, as the DIF form's does: each is clamped
    //      as it comes out of the butterfly, y0 included, by the argument given for x0 (nothing normalises in front of the clamp).
#pragma unroll
    for (int r = 0; r < 5; r++) {
      const int hb = 9 - 2 * r;                              // quarter distance D = 2^(hb - 1) = 256, 64, 16, 4, 1
      const u32 D = 1u << (hb - 1);
      const u32 m = q >> (hb - 1);                           // the quad's sub-block, < 4^r
      const u32 e0 = (m << (hb + 1)) | (q & (D - 1));
      const bool from_regs = DIRECT && r == 0;               // (e0 == tid, D == 256: the thread's own loads)
      LN<9> x0 = from_regs ? xin[0] : planes_get<FT>(lds, T, SWZ(e0));
      const LN<9> x1 = from_regs ? xin[1] : planes_get<FT>(lds, T, SWZ(e0 + D));
      const LN<9> x2 = from_regs ? xin[2] : planes_get<FT>(lds, T, SWZ(e0 + 2 * D)), x3 = from_regs ? xin[3] : planes_get<FT>(lds, T, SWZ(e0 + 3 * D));
      LN<9> p1, p2, p3;
      if (r < 2) {
        // round 0: one triple per tile; round 1: one per sub-block = per wave.  Scalar operands
        const u32 sb = r == 0 ? 0u : (u32)__builtin_amdgcn_readfirstlane(tid >> 6);
        const u32* wu = cls_pack + pi.u_off + ((u32)r * 4 + sb) * (3 * U_SLOT<FT>);
        mem_phase(false);
        if (!from_regs) ln::clamp_apply<FT>(x0, ln::clamp_row<FT>(nqp, ln::clamp_q<FT>(x0.v[8])));
        p2 = ln::mul_us<FT>(x2, wu + U_SLOT<FT>);
        p1 = ln::mul_us<FT>(x1, wu);
        p3 = ln::mul_us<FT>(x3, wu + 2 * U_SLOT<FT>);
      } else {
        const u32* blk = cls_pack + pi.round_off[r];
        const Tw<M2> w1 = tw_get<M2, 3>(blk, coset_sets(r), 0, 0, m), w2 = tw_get<M2, 3>(blk, coset_sets(r), 1, 0, m);
        const Tw<M2> w3 = tw_get<M2, 3>(blk, coset_sets(r), 2, 0, m);
        mem_phase(false);
        ln::clamp_apply<FT>(x0, ln::clamp_row<FT>(nqp, ln::clamp_q<FT>(x0.v[8])));
        p2 = tw_mul<M2>(x2, w2);
        p1 = tw_mul<M2>(x1, w1);
        p3 = tw_mul<M2>(x3, w3);
      }
      const LN<9> s02 = ln::add(x0, p2), d02 = ln::sub(x0, p2), s13 = ln::add(p1, p3);
      LN<9> y0 = ln::add(s02, s13), y1 = ln::sub(s02, s13);
      if (r < 4) ln::normalize<FT>(y0);
      const LN<9> t = ln::mul_us<FT>(ln::sub(p1, p3), a.wq_w);
      LN<9> y2 = ln::add(d02, t), y3 = ln::sub(d02, t);
      if (r == 0) { ln::normalize<FT>(y1); ln::normalize<FT>(y2); ln::normalize<FT>(y3); }
      mem_phase(true);
      if (r < 4) {
        planes_put<FT>(lds, T, SWZ(e0), y0);
        planes_put<FT>(lds, T, SWZ(e0 + D), y1);
        planes_put<FT>(lds, T, SWZ(e0 + 2 * D), y2);
        planes_put<FT>(lds, T, SWZ(e0 + 3 * D), y3);
        __syncthreads();
      } else {
        // D == 1: four consecutive elements of the row, |value| < 4.6p (M2: 9.04p), NOT normalised: y0's limbs lie in [0, 2^31 - 4] (a
        // clamped x0 plus three normalised products), those of y1, y2, y3 in (-2^30, 2^30) -- the two classes ln::clamp_apply takes as
        // they are (the bound the x0 of rounds 1 .. 4 goes by, above).  Clamp, pack, the rare conditional subtract, store
        u32* dstq = a.dst + (row * a.dst_stride + ((u64)tile << S)) * NL;          // (the tile; each element of the quad takes a scalar base of its own)
        clamp_store<FT, true>(lane_at(ubase(dstq + 0 * NL), e0 * (NL * 4u)), y0, nqp);
        clamp_store<FT, true>(lane_at(ubase(dstq + 1 * NL), e0 * (NL * 4u)), y1, nqp);
        clamp_store<FT, true>(lane_at(ubase(dstq + 2 * NL), e0 * (NL * 4u)), y2, nqp);
        clamp_store<FT, true>(lane_at(ubase(dstq + 3 * NL), e0 * (NL * 4u)), y3, nqp);
      }
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < SH::NR4; r++) {
    const int u = SH::U0 + 2 * r, hb = S - u - 1;            // stages (u, u + 1) of this pass; pair bit of stage u
    const bool last_two = LAST && (r == SH::NR4 - 1);        // stages k-2, k-1: twiddles 1, w^(n/4), 1
    const bool triv = NF && FIRST && (r == SH::NR4 - 1);     // pure form: the round with one twiddle set -- 1, 1, I
    const u32 lp = q & ((1u << LBT) - 1), j = q >> LBT;
    const u32 i0 = ((j >> (hb - 1)) << (hb + 1)) | (j & ((1u << (hb - 1)) - 1));
    const u32 e0 = (i0 << LBT) | lp;
    constexpr u32 one = 1u;
    const u32 dq = one << (hb - 1 + LBT);
    // quads q and q + period share their twiddles.  Pure form: the twiddles depend on the position in the sub-block alone, j mod 2^(hb - 1)
    const u32 period = NF ? one << (hb - 1) : one << (hb - 1 + LBT);
    const u32 jl = NF ? j & (period - 1) : q & (period - 1);
    const u32* blk = cls_pack + pi.round_off[SH::U0 + r];
    if (triv) {
      // ---- pure form, the last stage pair: c0 = b0 + b1, c1 = b0 - b1, c2, c3 = (x0 - x2) +- (x1 - x3) I.  Inputs: normalised,
      //      |value| < 2.7p (the uniform round before it: clamped sums and mul_u outputs; a lane-varying round: < 2.4p; loads and the
      //      radix-2 round's sums: < 2p), so |c0|, |c1| < 10.8p and |c2|, |c3| < 5.4p + 2.7p = 8.1p.  M2, S = 4, 5 (a lane-varying round
      //      straight before this one) and S = 3 (the radix-2 round's products): inputs < 3.01p, so |c0|, |c1| < 12.04p and |c2|, |c3| <
      //      6.02p + 2.7p = 8.72p -- the clamp takes |value| < 16p, the successor clamps x0 and multiplies the rest by mul_u.
      //      With the carries counted: c0, a sum of four normalised values, has limbs in [0, 2^31 - 4]; c1 = b0 - b1 (two sums of two) and
      //      c2, c3 = (x0 - x2) +- t have limbs in (-2^30, 2^30); |value| < 12.04p for all four -- ln::clamp_apply's two input classes.
      //      Packed intermediate (!MID): this round is the tile's last, and the quad is elements i = 4 j .. 4 j + 3 of column lp.  Each
      //      output is clamped ONCE, straight from its sum, packed and stored from the registers (ntt_ln_dev.h clamp_store): no
      //      normalise, no LDS round trip, no barrier, no store loop.  The lanes of consecutive lp store 2^LBT x 32 contiguous bytes,
      //      the segments the store loop wrote.
      //      Limb intermediate (MID): stored to LDS normalised, as before -- the successor's first round multiplies three of four by
      //      scalar operands (mul_u) -- and the plane-store loop below takes the tile
      const bool fr = DIRECT && SH::U0 == 0 && r == 0;       // S == 2: the thread's own loads
      const LN<9> x0 = fr ? xin[0] : planes_get<FT>(lds, T, SWZ(e0)), x1 = fr ? xin[1] : planes_get<FT>(lds, T, SWZ(e0 + dq));
      const LN<9> x2 = fr ? xin[2] : planes_get<FT>(lds, T, SWZ(e0 + 2 * dq)), x3 = fr ? xin[3] : planes_get<FT>(lds, T, SWZ(e0 + 3 * dq));
      mem_phase(false);
      const LN<9> b0 = ln::add(x0, x2), b1 = ln::add(x1, x3);
      LN<9> c0 = ln::add(b0, b1), c1 = ln::sub(b0, b1);
      const LN<9> b2 = ln::sub(x0, x2);
      const LN<9> t = ln::mul_us<FT>(ln::sub(x1, x3), a.wq_w);                                    // normalised, (-2p, 2.7p)
      LN<9> c2 = ln::add(b2, t), c3 = ln::sub(b2, t);
      if constexpr (!MID && SH::NR4 >= 1) {                  // (S == 1 has no such round: its instantiation keeps a single exit)
        if (RC < 0 && SH::U0 == 0 && canon) {
          // S == 2: no round before this one, every lane still holds Montgomery form: all four outputs are converted here
          ln::normalize<FT>(c0); ln::normalize<FT>(c1); ln::normalize<FT>(c2); ln::normalize<FT>(c3);
          c0 = ln::mul<FT>(c0, k32); c1 = ln::mul<FT>(c1, k32); c2 = ln::mul<FT>(c2, k32); c3 = ln::mul<FT>(c3, k32);
        }
        // S == 2: the storing round is the first round and no barrier has run yet; this one makes the q*p table, copied into LDS at
        // the kernel's top, visible to every wave before the first clamp reads it (the old route normalised c0 to stay off the table
        // and met the barrier behind its puts: one barrier then, one now)
        if constexpr (SH::U0 == 0 && SH::NR4 == 1) __syncthreads();
        mem_phase(true);
        u32* dstq = ubase(a.dst + row * a.dst_stride * NL);
        clamp_store<FT, false>(lane_at(dstq, gindex(e0) * (NL * 4u)), c0, nqp);     // [0, p + 2^239) < 2^256: what the successor reads
        clamp_store<FT, false>(lane_at(dstq, gindex(e0 + dq) * (NL * 4u)), c1, nqp);
        clamp_store<FT, false>(lane_at(dstq, gindex(e0 + 2 * dq) * (NL * 4u)), c2, nqp);
        clamp_store<FT, false>(lane_at(dstq, gindex(e0 + 3 * dq) * (NL * 4u)), c3, nqp);
        return;
      }
      ln::normalize<FT>(c1); ln::normalize<FT>(c2); ln::normalize<FT>(c3);
      if (RC < 0 && SH::U0 == 0 && canon) {
        // S == 2: no round before this one, every lane still holds Montgomery form: all four outputs are converted here
        ln::normalize<FT>(c0);
        c0 = ln::mul<FT>(c0, k32); c1 = ln::mul<FT>(c1, k32); c2 = ln::mul<FT>(c2, k32); c3 = ln::mul<FT>(c3, k32);
      } else if (fr) {
        ln::normalize<FT>(c0);                                                                  // (a sum of four loads: < 4.01p)
      } else {
        ln::clamp_apply<FT>(c0, ln::clamp_row<FT>(nqp, ln::clamp_q<FT>(c0.v[8])));
      }
      planes_put<FT>(lds, T, SWZ(e0), c0);
      planes_put<FT>(lds, T, SWZ(e0 + dq), c1);
      planes_put<FT>(lds, T, SWZ(e0 + 2 * dq), c2);
      planes_put<FT>(lds, T, SWZ(e0 + 3 * dq), c3);
      mem_phase(true);
      __syncthreads();
      continue;
    }
    if constexpr (RU >= 0) {
      if (r >= RU && !last_two) {
        // ---- a uniform round: wave w takes the quads q = w mod 4, whose twiddles are the three of pack slot (w): scalar operands.
        //      Block 0 is gone (converted in round RU - 1), so every lane multiplies by the same plain constants.
        const u32 wv = __builtin_amdgcn_readfirstlane(tid >> 6);
        // pure form: the twiddles go by j mod 4, so wave w takes the quads j = 4 m + w, (m, lp) = the lane
        const u32 qu = NF ? (((((tid & 63u) >> LBT) << 2) | wv) << LBT) | (tid & ((1u << LBT) - 1)) : ((tid & 63u) << 2) | wv;
        const u32 lpu = qu & ((1u << LBT) - 1), ju = qu >> LBT;
        const u32 iu = ((ju >> (hb - 1)) << (hb + 1)) | (ju & ((1u << (hb - 1)) - 1));
        const u32 eu = (iu << LBT) | lpu;
        const u32* wu = cls_pack + pi.u_off + ((r - RU) * 4 + wv) * (3 * U_SLOT<FT>);
        const LN<9> x0 = planes_get<FT>(lds, T, SWZ(eu)), x1 = planes_get<FT>(lds, T, SWZ(eu + dq));
        const LN<9> x2 = planes_get<FT>(lds, T, SWZ(eu + 2 * dq)), x3 = planes_get<FT>(lds, T, SWZ(eu + 3 * dq));
        mem_phase(false);
        const LN<9> b0 = ln::add(x0, x2), b1 = ln::add(x1, x3);
        LN<9> c0 = ln::add(b0, b1);
        ln::clamp_apply<FT>(c0, ln::clamp_row<FT>(nqp, ln::clamp_q<FT>(c0.v[8])));
        planes_put<FT>(lds, T, SWZ(eu), c0);
        LN<9> d1 = ln::sub(b0, b1);
        ln::normalize<FT>(d1);                                                                 // mul_u wants sum |limb| < 9 * 2^29
        planes_put<FT>(lds, T, SWZ(eu + dq), ln::mul_us<FT>(d1, wu + 2 * U_SLOT<FT>));
        const LN<9> b2 = ln::mul_us<FT>(ln::sub(x0, x2), wu);
        const LN<9> b3 = ln::mul_us<FT>(ln::sub(x1, x3), wu + U_SLOT<FT>);                            // (-2p, 2.7p)
        LN<9> c2 = ln::add(b2, b3);
        // (pure form: clamped, (-4p, 5.4p) -> [0, p + 2^239), so that the I-only round after it adds four values below 2.7p)
        // (DIF form, a first pass that stores the limb intermediate: clamped as well.  The sum of two mul_u products lies in (-4p, 5.4p),
        // which is fine for the rounds of this tile -- their sums are clamped -- but not for a record: invariant I, |value| < 4p, is
        // what the successor's first round is built for, and a uniform round is this pass's last)
        if constexpr (NF || (FIRST && MID)) ln::clamp_apply<FT>(c2, ln::clamp_row<FT>(nqp, ln::clamp_q<FT>(c2.v[8])));
        else ln::normalize<FT>(c2);
        planes_put<FT>(lds, T, SWZ(eu + 2 * dq), c2);
        planes_put<FT>(lds, T, SWZ(eu + 3 * dq), ln::mul_us<FT>(ln::sub(b2, b3), wu + 2 * U_SLOT<FT>));
        mem_phase(true);
        __syncthreads();
        continue;
      }
    }
    if (u == 0 && zero_hi) {                                 // (pure form, S == 2: the I-only round above took it, zeros and all)
      // zero-padded first round (rate <= 1/2): x2 = x3 = 0, the stage-0 butterflies are (x, x w); inputs < p; everything
      // is block 0, so with canonical output the three multiplies leaving it (w0, w3, and w2 for c1) take the converting set
      const u32 vb = canon ? 3u : 0u;
      const Tw<M2> w0 = tw_get<M2, 6>(blk, period, 0, vb, jl), w3 = tw_get<M2, 6>(blk, period, 1, vb, jl), w2 = tw_get<M2, 6>(blk, period, 2, vb, jl);
      mem_phase(false);
      const bool cv0 = NF && canon && r == RC;               // pure form: the round that converts the pure sum as well (below)
      if (n_val <= (1u << (k - 2))) {                  // rate <= 1/4: x1 is zero too
        const LN<9> x0 = DIRECT ? xin[0] : planes_get<FT>(lds, T, SWZ(e0));
        if constexpr (DIRECT) planes_put<FT>(lds, T, SWZ(e0), cv0 ? ln::mul<FT>(x0, k32) : x0);
        planes_put<FT>(lds, T, SWZ(e0 + dq), tw_mul<M2>(x0, w2));
        planes_put<FT>(lds, T, SWZ(e0 + 2 * dq), tw_mul<M2>(x0, w0));
        planes_put<FT>(lds, T, SWZ(e0 + 3 * dq), tw_mul<M2>(x0, w3));
      } else {
        const LN<9> x0 = DIRECT ? xin[0] : planes_get<FT>(lds, T, SWZ(e0)), x1 = DIRECT ? xin[1] : planes_get<FT>(lds, T, SWZ(e0 + dq));
        LN<9> c0 = ln::add(x0, x1);                                                           // [0, 2p)
        ln::normalize<FT>(c0);
        planes_put<FT>(lds, T, SWZ(e0), cv0 ? ln::mul<FT>(c0, k32) : c0);
        planes_put<FT>(lds, T, SWZ(e0 + dq), tw_mul<M2>(ln::sub(x0, x1), w2));
        const LN<9> t = ln::mul_us<FT>(x1, a.wq_w);                                                // x1 I (plain constant: t keeps x1's form); (-2p, 2.7p)
        planes_put<FT>(lds, T, SWZ(e0 + 2 * dq), tw_mul<M2>(ln::add(x0, t), w0));                   // in: limbs (-2^29, 2^30), |value| < 3.7p
        planes_put<FT>(lds, T, SWZ(e0 + 3 * dq), tw_mul<M2>(ln::sub(x0, t), w3));
      }
      mem_phase(true);
      __syncthreads();
      continue;
    }
    const bool from_regs = DIRECT && SH::U0 == 0 && r == 0;   // (e0 == tid, dq == 256: the thread's own loads)
    const LN<9> x0 = from_regs ? xin[0] : planes_get<FT>(lds, T, SWZ(e0)), x1 = from_regs ? xin[1] : planes_get<FT>(lds, T, SWZ(e0 + dq));
    const LN<9> x2 = from_regs ? xin[2] : planes_get<FT>(lds, T, SWZ(e0 + 2 * dq)), x3 = from_regs ? xin[3] : planes_get<FT>(lds, T, SWZ(e0 + 3 * dq));     // I: normalised, |value| < 4p
    mem_phase(false);
    const LN<9> b0 = ln::add(x0, x2), b1 = ln::add(x1, x3);                                   // limbs [0, 2^30), |value| < 8p
    LN<9> c0 = ln::add(b0, b1);                                                               // limbs [0, 2^31), |value| < 16p
    if (last_two) {
      // outputs go straight to the store path, as the sums leave them: c0 limbs [0, 2^31 - 4], c1, c2, c3 limbs (-2^30, 2^30) (b0 - b1: two
      // sums of two normalised values; (x0 - x2) +- b3: a difference of two and a normalised product), |value| < 16p -- ln::clamp_apply's
      // two input classes; its carry pass is the only one they get
      LN<9> c1 = ln::sub(b0, b1);
      const LN<9> b2 = ln::sub(x0, x2);
      // w^(n/4) is the one twiddle every lane shares: its multiply takes the shifted-multiples form (scalar operands)
      const LN<9> b3 = ln::mul_us<FT>(ln::sub(x1, x3), a.wq_w);
      LN<9> c2 = ln::add(b2, b3);
      LN<9> c3 = ln::sub(b2, b3);
      // dq == 1 here: the quad is four CONSECUTIVE elements of the row, 128 bytes -- reduced and stored from the registers (no LDS round
      // trip, no barrier; -0.2 ... -0.8 % by shape).  -> [0, p): ntt_ln_dev.h clamp_store
      mem_phase(true);
      u32* dstq = a.dst + (row * a.dst_stride + ((u64)tile << S)) * NL;          // (the tile; each element of the quad takes a scalar base of its own)
      clamp_store<FT, true>(lane_at(ubase(dstq + 0 * NL), e0 * (NL * 4u)), c0, nqp);
      clamp_store<FT, true>(lane_at(ubase(dstq + 1 * NL), e0 * (NL * 4u)), c1, nqp);
      clamp_store<FT, true>(lane_at(ubase(dstq + 2 * NL), e0 * (NL * 4u)), c2, nqp);
      clamp_store<FT, true>(lane_at(ubase(dstq + 3 * NL), e0 * (NL * 4u)), c3, nqp);
      return;
    } else {
      // clamp the pure sum at once: c0 leaves the registers before the multiplier chains start (holding it and its
      // q*p row across them spills at 128 VGPRs: +1 GB of scratch writes per pass, profiles/r02b)
      // (a first round fed by the loads: four values < p + 2^239, their sum < 4.001 p needs the carries only -- and no q*p table yet)
      if (from_regs) ln::normalize<FT>(c0);
      else ln::clamp_apply<FT>(c0, ln::clamp_row<FT>(nqp, ln::clamp_q<FT>(c0.v[8])));                  // [0, p + 2^239)
      planes_put<FT>(lds, T, SWZ(e0), c0);
      // block 0 of stages (u, u + 1) = the quads whose elements all lie below n / 2^(t + 2): here exactly q < period in the
      // tiles that hold block 0.  Their three multiplies that leave block 0 (c1, c2, c3) take the converting set; c0 stays a
      // pure sum
      // Pure form: block 0 of a column is i < 2^(S - u - 2), the quads q < dq of EVERY tile, through round RC (every round that comes
      // here), which converts c0 too: after it every slot is canonical -- c1, c2, c3 of the block-0 quads of rounds <= RC by their
      // converting twiddles, c0 of round RC by 2^5, and everything else descends from those
      const bool blk0c = NF ? canon && q < dq : canon && blk0_tile && q < period && (RU < 0 || r < RU);
      if constexpr (NF ? RC >= 0 : RU >= 1) {
        if (r == (NF ? RC : RU - 1) && blk0c) {
          // the last round before the uniform one: c0, the pure sum that would carry block 0 on, is converted as well (a multiply
          // by 2^5 = 2^261 R^-1: 16 lanes of one wave per block-0 tile; pure form: the lanes q < dq), so that the uniform round sees
          // canonical values only
          planes_put<FT>(lds, T, SWZ(e0), ln::mul<FT>(c0, k32));
        }
      }
      const u32 vb = blk0c ? 3u : 0u;
      if constexpr (M2) {
        // the same butterfly as below on 18 words per twiddle: w3's are asked for behind the first product, under whose chain they
        // arrive, and the two differences are taken before it, so that x0 .. x3 are dead when the first chain starts (all three pairs
        // up front spill at 128 VGPRs)
        const Tw<M2> w2 = tw_get<M2, 6>(blk, period, 2, vb, jl), w0 = tw_get<M2, 6>(blk, period, 0, vb, jl);
        const LN<9> d1 = ln::sub(b0, b1);
        const LN<9> d13 = ln::sub(x1, x3), e2 = ln::sub(x0, x2);
        planes_put<FT>(lds, T, SWZ(e0 + dq), tw_mul<M2>(d1, w2));                                   // normalised, (-3.01p, 2.01p)
        __builtin_amdgcn_sched_barrier(0);
        const Tw<M2> w3 = tw_get<M2, 6>(blk, period, 1, vb, jl);
        const LN<9> t = ln::mul_us<FT>(d13, a.wq_w);                                                // normalised, (-2p, 2.7p)
        planes_put<FT>(lds, T, SWZ(e0 + 2 * dq), tw_mul<M2>(ln::add(e2, t), w0));
        planes_put<FT>(lds, T, SWZ(e0 + 3 * dq), tw_mul<M2>(ln::sub(e2, t), w3));
      } else {
      const Tw<M2> w0 = tw_get<M2, 6>(blk, period, 0, vb, jl), w3 = tw_get<M2, 6>(blk, period, 1, vb, jl);
      const Tw<M2> w2 = tw_get<M2, 6>(blk, period, 2, vb, jl);
      const LN<9> d1 = ln::sub(b0, b1);                                                       // limbs (-2^30, 2^30), |value| < 16p
      planes_put<FT>(lds, T, SWZ(e0 + dq), tw_mul<M2>(d1, w2));                                     // normalised, (-1.2p, 0.2p]
      // t = (x1 - x3) I by the plain constant: in block 0 it stays in the form of its inputs and the two products below convert
      const LN<9> t = ln::mul_us<FT>(ln::sub(x1, x3), a.wq_w);                                     // normalised, (-2p, 2.7p)
      const LN<9> e2 = ln::sub(x0, x2);                                                       // limbs (-2^29, 2^29), |value| < 8p
      planes_put<FT>(lds, T, SWZ(e0 + 2 * dq), tw_mul<M2>(ln::add(e2, t), w0));                     // in: limbs (-2^29, 2^30), |value| < 10.7p
      planes_put<FT>(lds, T, SWZ(e0 + 3 * dq), tw_mul<M2>(ln::sub(e2, t), w3));
      }
    }
    mem_phase(true);                                         // the barrier, then the next round's reads and twiddle loads (or the store phase)
    __syncthreads();
  }

  if constexpr (FIRST && MID) {
    // DIF form: every slot holds a normalised value with |value| < 4p (c0 clamped, c1 / c3 products, c2 a normalised sum of two
    // products; after a lone radix-2 round: loads, normalised sums, products).  Pure form: the I-only round's outputs, normalised,
    // c0 clamped, |c1| < 10.8p (12.04p behind an ln::mul2 round), |c2|, |c3| < 8.72p -- NOT invariant I; the coset pass clamps x0 and
    // multiplies the rest by mul_u (tests/test_gpu_k1_passes.py holds the records to 12.04p).  Stored as it is.  lb == 10 (the successor
    // runs 10 stages), so slot (i, lp) is element (tile << LTJ | lp) of the successor's tile i
    u32* mrow = ubase(a.mid + (row << k) * 9);
    // (the lane offsets are formed afresh from the thread index: shared with the tile load's, they would sit in registers across
    // every round -- scratch at 128 VGPRs for S = 9)
    u32 tid_st = tid;
    asm volatile("" : "+v"(tid_st));
#pragma unroll
    for (u32 e = tid_st; e < T; e += 256) {
      const u32 e2 = (tile << LTJ) | (e & ((1u << LBT) - 1));
      const u32 t = (e >> LBT) * (9 * T * 4u);                // byte offset of the successor's tile in this row: < 2^S * 36 KiB
      const LN<9> x = planes_get<FT>(lds, T, SWZ(e));
      *reinterpret_cast<uint4*>(lane_at(mrow, t + e2 * 16u)) = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
      *reinterpret_cast<uint4*>(lane_at(mrow, t + (T + e2) * 16u)) = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
      *lane_at(mrow, t + (8 * T + e2) * 4u) = x.v[8];
    }
    return;
  }
  if constexpr (FIRST) {           // (a last pass has stored from its final round and returned)
  u32* dst = ubase(a.dst + row * a.dst_stride * NL);
  u32 tid_st = tid;                                          // (as for the limb intermediate's store above)
  asm volatile("" : "+v"(tid_st));
#pragma unroll
  for (u32 e = tid_st; e < T; e += 256) {
    const u32 g = gindex(e);
    LN<9> x = planes_get<FT>(lds, T, SWZ(e));                                        // normalised, |value| < 16p
    ln::clamp_apply<FT>(x, ln::clamp_row<FT>(nqp, ln::clamp_q<FT>(x.v[8])));        // [0, p + 2^239) < 2^256: what the successor reads as limbs anyway
    u32 w[8];
    ln::to_packed<FT>(w, x.v);
    Fe<NL> v;
#pragma unroll
    for (int i = 0; i < 8; i++) v.v[i] = w[i];
    fe_store<NL>(lane_at(dst, g * (NL * 4u)), v);
  }
  }
}

template <int S, int LTJ, bool FIRST, bool MID, bool NF, bool M2>
hipError_t launch_tm(const NttPassArgs& a, const u32* pack, const NttPackInfo& pi, hipStream_t st) {
  constexpr int LT = S + LTJ;
  const u64 tiles = ((u64)1 << (a.log_n - LT)) * a.n_rows;
  const size_t lds_bytes = (((size_t)1 << LT) * 9 + 64 * LnField<FT255>::STRIDE) * 4;   // tile + q*p table
  // hipFuncSetAttribute is idempotent and cheap; calling it on every launch keeps this free of unsynchronised caches
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ntt_pass_l9s_kernel<S, LTJ, FIRST, MID, NF, M2>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((ntt_pass_l9s_kernel<S, LTJ, FIRST, MID, NF, M2>), dim3((unsigned)tiles), dim3(256), lds_bytes, st, a, pack, pi);
  return hipGetLastError();
}
template <int S, int LTJ, bool FIRST>
hipError_t launch_t(const NttPassArgs& a, const u32* pack, const NttPackInfo& pi, hipStream_t st) {
  if (pi.mul2) {
    // the split packs exist for the pure / coset form only, and only for the passes that ntt_l9s_mul2_supported names
    if constexpr (ntt_l9s_mul2_supported(S, FIRST)) { if (a.form) return a.mid ? launch_tm<S, LTJ, FIRST, true, true, true>(a, pack, pi, st) : launch_tm<S, LTJ, FIRST, false, true, true>(a, pack, pi, st); }
    return hipErrorInvalidValue;
  }
  if (a.form) return a.mid ? launch_tm<S, LTJ, FIRST, true, true, false>(a, pack, pi, st) : launch_tm<S, LTJ, FIRST, false, true, false>(a, pack, pi, st);
  return a.mid ? launch_tm<S, LTJ, FIRST, true, false, false>(a, pack, pi, st) : launch_tm<S, LTJ, FIRST, false, false, false>(a, pack, pi, st);
}

}  // namespace

bool ntt_l9s3_supported(uint32_t log_n) { return log_n >= 21 && log_n <= 26; }

bool ntt_l9s_supported(uint32_t log_n, uint32_t n_passes, int log_tile) { return n_passes == 2 && log_tile == 10 && log_n >= 11 && log_n <= 20; }

#define L9S_FIRST_CASES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10)

hipError_t launch_ntt_pass_l9s(const NttPassArgs& a, bool first, const uint32_t* pack, const NttPackInfo& pi, hipStream_t st) {
  if (!first) {
    if (a.s != 10 || a.log_tj != 0 || a.t0 + a.s != a.log_n) return hipErrorInvalidValue;
    // (the last pass has a uniform round and converts block 0 before it: no Montgomery-form prefix is left for the store to reduce)
    if (a.mont_prefix) return hipErrorInvalidValue;
    return launch_t<10, 0, false>(a, pack, pi, st);
  }
  // two-pass plans: s + 10 stages in all; three-pass plans: s + 20 (the first pass works at element stride 2^20)
  if (a.t0 != 0 || a.s + a.log_tj != 10 || (a.s + 10 != a.log_n && a.s + 20 != a.log_n)) return hipErrorInvalidValue;
  if (a.form && a.s + 10 != a.log_n) return hipErrorInvalidValue;      // (the pure / coset form: two-pass plans only)
  // a first pass addresses its row by 32-bit byte offsets from the row's start (the kernel's "Global addresses"): 2^26 columns x 32 B
  // = 2^31 is the largest plan there is (ntt_l9s3_supported); a wider row would wrap
  if (a.log_n > 26) return hipErrorInvalidValue;
  if (a.tile_group && ((1u << (a.log_n - 10)) >> a.tile_group) < 8) return hipErrorInvalidValue;
  switch (a.s) {
#define X(SV) case SV: return launch_t<SV, 10 - SV, true>(a, pack, pi, st);
    L9S_FIRST_CASES(X)
#undef X
  }
  return hipErrorInvalidValue;
}

}  // namespace lcpc
