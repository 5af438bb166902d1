// lcpc_amd/csrc/ints.cpp -- the plain-integer extension of the C ABI (include/lcpc_hip_ints.h): integers -> field elements on the host
// (host_field.h, no HIP call) and on the device (K9, ints.hip), and the two commit entry points that read integers.  The commit
// pipelines themselves are commit.cpp's: commit_host_locked is lcpc_commit's own loop with another source, commit_ints_device_locked
// the resident path behind K9.
#include "internal.h"
#include "../../include/lcpc_hip_ints.h"

using namespace lcpc;

static_assert(LCPCI_U32 == INTS_U32 && LCPCI_I32 == INTS_I32 && LCPCI_U64 == INTS_U64 && LCPCI_I64 == INTS_I64 && LCPCI_WIDE == INTS_WIDE,
              "lcpci_kind and the launcher's kinds are one numbering");

namespace {

inline bool kind_ok(uint32_t kind) { return kind <= LCPCI_WIDE; }

// the input's natural alignment (WIDE: that of a limb)
inline bool in_aligned(const void* p, uint32_t kind, int L) {
  const size_t ib = ints_elem_bytes((int)kind, L);
  return reinterpret_cast<uintptr_t>(p) % (ib < 8 ? ib : 8) == 0;
}

// one integer -> o = (v mod p) R mod p.  The magnitude goes into h_mul as it is: the product a R^2 < 2^(64 L) p and the L reduction
// rounds leave (a R^2 + m p) / R < 2p for every a < 2^(64 L), which h_mul's one subtraction brings below p.  A negative v is
// p - (|v| R mod p), 0 for 0 (h_sub from zero).  |v| is taken in unsigned arithmetic: -2^31 and -2^63 have no positive counterpart
// at their own width
void from_int(const FieldDesc& f, uint32_t kind, const uint8_t* in, uint64_t* o) {
  uint64_t a[MAXL] = {0, 0, 0, 0};
  bool neg = false;
  switch (kind) {
    case LCPCI_U32: { uint32_t w; memcpy(&w, in, 4); a[0] = w; break; }
    case LCPCI_I32: {
      uint32_t w;
      memcpy(&w, in, 4);
      neg = (w >> 31) != 0;
      a[0] = neg ? (uint32_t)(0u - w) : w;
      break;
    }
    case LCPCI_U64: memcpy(&a[0], in, 8); break;
    case LCPCI_I64: {
      uint64_t w;
      memcpy(&w, in, 8);
      neg = (w >> 63) != 0;
      a[0] = neg ? (uint64_t)0 - w : w;
      break;
    }
    default: memcpy(a, in, 8 * (size_t)f.L); break;
  }
  h_mul(f, o, a, f.r2);
  if (neg) {
    const uint64_t zero[MAXL] = {0, 0, 0, 0};
    h_sub(f, o, zero, o);
  }
}

}  // namespace

extern "C" {

int lcpci_version(void) { return LCPCI_VERSION; }

int lcpci_from_ints(uint32_t field, uint32_t kind, const void* in, uint64_t n, uint64_t* out_mont) {
  const FieldDesc* f = field_desc((int)field);
  if (!f || !kind_ok(kind)) return LCPC_ERR_ARG;
  if (n == 0) return 0;
  if (!in || !out_mont) return LCPC_ERR_ARG;
  const size_t ib = ints_elem_bytes((int)kind, f->L);
  const uint8_t* p = static_cast<const uint8_t*>(in);
  for (uint64_t i = 0; i < n; i++) from_int(*f, kind, p + i * ib, out_mont + i * f->L);
  return 0;
}

int lcpci_to_canon(uint32_t field, const uint64_t* in_mont, uint64_t n, uint64_t* out_canon) {
  const FieldDesc* f = field_desc((int)field);
  if (!f) return LCPC_ERR_ARG;
  if (n == 0) return 0;
  if (!in_mont || !out_canon) return LCPC_ERR_ARG;
  for (uint64_t i = 0; i < n; i++) h_canon(*f, out_canon + i * f->L, in_mont + i * f->L);
  return 0;
}

int lcpci_from_ints_device(lcpc_ctx* c, uint32_t kind, const void* in_dev, uint64_t n, uint64_t* out_dev, void* stream) {
  if (!c || !in_dev || !out_dev || n == 0 || !kind_ok(kind)) return LCPC_ERR_ARG;
  if (!in_aligned(in_dev, kind, c->L) || reinterpret_cast<uintptr_t>(out_dev) % (c->L % 2 ? 8 : 16)) return LCPC_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->prm.device));
  HIPCHK(c, launch_from_ints(c->NL, (int)kind, in_dev, n, c->d_r2, reinterpret_cast<uint32_t*>(out_dev), (hipStream_t)stream));
  return 0;
}

int lcpci_commit_ints_device(lcpc_commit_t* m, uint32_t kind, const void* vals_dev, uint64_t n, void* stream, uint8_t* root) {
  if (!m || !vals_dev || n == 0 || !kind_ok(kind)) return LCPC_ERR_ARG;
  const lcpc_ctx* c = m->enc;
  if (!in_aligned(vals_dev, kind, c->L)) return LCPC_ERR_ARG;
  if (c->prm.shard_count > 1) return LCPC_ERR_STATE;
  LCPC_TRY
  std::unique_lock<FillLock> fill(m->fill_mu);      // a fill: waits for the readers in flight (internal.h)
  std::lock_guard<std::mutex> g(m->mu);
  HIPCHK(m, hipSetDevice(c->prm.device));
  return commit_ints_device_locked(m, (int)kind, vals_dev, n, (hipStream_t)stream, root);
  LCPC_CATCH(m)
}

int lcpci_commit_ints(lcpc_commit_t* m, uint32_t kind, const void* vals_host, uint64_t n, uint8_t* root) {
  if (!m || !vals_host || n == 0 || !kind_ok(kind)) return LCPC_ERR_ARG;
  const lcpc_ctx* c = m->enc;
  if (c->prm.shard_count > 1) return LCPC_ERR_STATE;
  LCPC_TRY
  std::unique_lock<FillLock> fill(m->fill_mu);
  std::lock_guard<std::mutex> g(m->mu);
  HIPCHK(m, hipSetDevice(c->prm.device));
  return commit_host_locked(m, HostSource{vals_host, (int)kind}, n, root);
  LCPC_CATCH(m)
}

}  // extern "C"
