// lcpc_amd/csrc/ints.hip -- K9: plain integers -> Montgomery-form field elements (include/lcpc_hip_ints.h).
//
// One element per lane, the grid sized to n (64-bit index; no grid-stride loop, so no element count takes a path of its own).
// A lane reads its integer at the element's natural alignment -- 4 bytes, 8 bytes, or L x 8 bytes; neighbouring lanes read
// neighbouring elements, so a wave reads one contiguous run -- takes the magnitude of a negative value in unsigned arithmetic,
// multiplies by R^2 and stores the element as to_mont_kernel (kernels.hip) does: 4 NL contiguous bytes per lane in 16-byte moves
// (8-byte for Ft63 / Ft191), lane i next to lane i + 1.
//
// The multiply is fe_mul (field_dev.h), whose CIOS loop does not need its FIRST operand below p: with the invariant t < 2p in front
// of a round, t' = (t + a_i b + m p) / 2^32 < (2p + (2^32 - 1) p + (2^32 - 1) p) / 2^32 = 2p for ANY limb a_i < 2^32 and b < p, and
// t + a_i b + m p < 2^32 (2p) < 2^(32 NL + 32) stays inside the NL + 2 words it is summed in (p < 2^(32 NL - 1) in all four fields).
// So fe_mul(a, R^2) is a R mod p, fully reduced after the one conditional subtraction, for every a < 2^(32 NL) -- which is why
// a 64-bit value into Ft63 (p < 2^63) and a WIDE value into any field go into the multiply as they are.
#include "kernels.h"
#include "field_dev.h"

namespace lcpc {

namespace {

template <int NL, int KIND>
__global__ void __launch_bounds__(256) from_ints_kernel(const void* in, u64 n, const u32* r2, u32* out, bool in16) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Fe<NL> a = fe_zero<NL>();
  bool neg = false;
  if constexpr (KIND == INTS_U32 || KIND == INTS_I32) {
    u32 w = static_cast<const u32*>(in)[i];
    if constexpr (KIND == INTS_I32) {
      neg = (w >> 31) != 0;
      if (neg) w = 0u - w;                // -2^31 has no positive counterpart in 32 signed bits: its magnitude is 2^31, unsigned
    }
    a.v[0] = w;
  } else if constexpr (KIND == INTS_U64 || KIND == INTS_I64) {
    const uint2 t = static_cast<const uint2*>(in)[i];
    u64 w = ((u64)t.y << 32) | t.x;
    if constexpr (KIND == INTS_I64) {
      neg = (w >> 63) != 0;
      if (neg) w = (u64)0 - w;            // likewise -2^63
    }
    a.v[0] = (u32)w; a.v[1] = (u32)(w >> 32);
  } else {
    // WIDE: NL / 2 limbs of 64 bits.  16-byte loads only where the input is 16-byte aligned (uniform for the launch) and the element a
    // multiple of 16 bytes; else 8-byte loads, the alignment the interface asks for
    const u32* p = static_cast<const u32*>(in) + i * NL;
    if (NL % 4 == 0 && in16) {
      a = fe_load<NL>(p);
    } else {
      const uint2* q = reinterpret_cast<const uint2*>(p);
#pragma unroll
      for (int k = 0; k < NL / 2; k++) {
        const uint2 t = q[k];
        a.v[2 * k] = t.x; a.v[2 * k + 1] = t.y;
      }
    }
  }
  Fe<NL> r = fe_mul<NL>(a, fe_load<NL>(r2));     // a < 2^(32 NL), R^2 < p: the bound above
  if (neg) r = fe_sub<NL>(fe_zero<NL>(), r);     // p - r, and 0 for r = 0
  fe_store<NL>(out + i * NL, r);
}

template <int NL> void launch_kind(int kind, dim3 grid, hipStream_t st, const void* in, u64 n, const u32* r2, u32* out, bool in16) {
  switch (kind) {
    case INTS_U32: hipLaunchKernelGGL((from_ints_kernel<NL, INTS_U32>), grid, dim3(256), 0, st, in, n, r2, out, in16); break;
    case INTS_I32: hipLaunchKernelGGL((from_ints_kernel<NL, INTS_I32>), grid, dim3(256), 0, st, in, n, r2, out, in16); break;
    case INTS_U64: hipLaunchKernelGGL((from_ints_kernel<NL, INTS_U64>), grid, dim3(256), 0, st, in, n, r2, out, in16); break;
    case INTS_I64: hipLaunchKernelGGL((from_ints_kernel<NL, INTS_I64>), grid, dim3(256), 0, st, in, n, r2, out, in16); break;
    default: hipLaunchKernelGGL((from_ints_kernel<NL, INTS_WIDE>), grid, dim3(256), 0, st, in, n, r2, out, in16); break;
  }
}

}  // namespace

hipError_t launch_from_ints(int nl, int kind, const void* in, u64 n, const u32* r2, u32* out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if ((nl != 2 && nl != 4 && nl != 6 && nl != 8) || kind < INTS_U32 || kind > INTS_WIDE) return hipErrorInvalidValue;
  const size_t ib = ints_elem_bytes(kind, nl / 2);
  const uintptr_t ia = reinterpret_cast<uintptr_t>(in), oa = reinterpret_cast<uintptr_t>(out);
  if (ia % (ib < 8 ? ib : 8) || oa % (nl % 4 == 0 ? 16 : 8)) return hipErrorInvalidValue;      // (fe_store's moves)
  const u64 blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;        // grid.x
  const dim3 grid((unsigned)blocks);
  const bool in16 = ia % 16 == 0;
  switch (nl) {
    case 2: launch_kind<2>(kind, grid, st, in, n, r2, out, in16); break;
    case 4: launch_kind<4>(kind, grid, st, in, n, r2, out, in16); break;
    case 6: launch_kind<6>(kind, grid, st, in, n, r2, out, in16); break;
    default: launch_kind<8>(kind, grid, st, in, n, r2, out, in16); break;
  }
  return hipGetLastError();
}

}  // namespace lcpc
