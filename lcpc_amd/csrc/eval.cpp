// lcpc_amd/csrc/eval.cpp -- the evaluation extension of the C ABI (include/lcpc_hip_eval.h): the tensors of an opening from a point,
// on the host (host_field.h, no HIP call) and on the device (K10, eval.hip), the field dot product (K11) and the value of a committed
// polynomial at points.  The collapse is commit.cpp's collapse_run as it is; this file adds what stands in front of it (K10) and
// behind it (K11) and the scratch layout around the three.
#include "internal.h"
#include "../../include/lcpc_hip_eval.h"

using namespace lcpc;

static_assert(LCPCE_POWERS == EVAL_POWERS && LCPCE_ML_MONOMIAL == EVAL_ML_MONOMIAL && LCPCE_ML_LAGRANGE == EVAL_ML_LAGRANGE,
              "lcpce_basis and the launcher's bases are one numbering");

namespace {

constexpr uint32_t MAX_POINTS = 65535;      // the expansion's second grid dimension

inline unsigned bit_len(uint64_t v) { return v ? 64u - (unsigned)__builtin_clzll(v) : 0u; }
inline bool pow2(uint64_t v) { return v && !(v & (v - 1)); }
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// What a basis makes of a shape: the pairs per point in K10's table, and which of them each tensor reads
struct Shape {
  uint32_t tab_bits = 0;           // pairs (lo_k, hi_k) per point
  uint32_t in_bits = 0;            // inner: pairs [0, in_bits), index j
  uint32_t out_first = 0, out_bits = 0;   // outer: pairs [out_first, out_first + out_bits), index r * out_stride
  uint64_t out_stride = 1;
};
// LCPC_ERR_ARG for an unknown basis, an empty dimension, a largest exponent that overflows, an n_point that does not fit
int shape_of(uint32_t basis, uint32_t n_point, uint64_t n_rows, uint64_t n_per_row, Shape* s) {
  if (basis > LCPCE_ML_LAGRANGE || n_rows == 0 || n_per_row == 0) return LCPC_ERR_ARG;
  if (n_rows - 1 > ~(uint64_t)0 / n_per_row) return LCPC_ERR_ARG;
  *s = Shape{};
  if (basis == LCPCE_POWERS) {
    if (n_point != 1) return LCPC_ERR_ARG;
    s->in_bits = bit_len(n_per_row - 1);
    s->out_bits = bit_len((n_rows - 1) * n_per_row);
    s->out_stride = n_per_row;
    s->tab_bits = std::max(s->in_bits, s->out_bits);
    return 0;
  }
  if (!pow2(n_rows) || !pow2(n_per_row)) return LCPC_ERR_ARG;
  s->in_bits = bit_len(n_per_row - 1);
  s->out_first = s->in_bits;
  s->out_bits = bit_len(n_rows - 1);
  s->tab_bits = s->in_bits + s->out_bits;
  return n_point == s->tab_bits ? 0 : LCPC_ERR_ARG;
}

bool all_reduced(const FieldDesc& f, const uint64_t* e, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    if (h_ge_p(f, e + i * f.L)) return false;
  return true;
}

// out[i] = product over k of (bit k of i ? hi[k] : lo[k]) for i < n, by doubling: one multiplication per element (two with lo).
// hi / lo: [bit_len(n - 1)][L]; lo == nullptr: every lo[k] is 1
void expand_host(const FieldDesc& f, const uint64_t* hi, const uint64_t* lo, uint64_t n, uint64_t* out) {
  const int L = f.L;
  memcpy(out, f.r, 8 * L);
  for (unsigned k = 0; k < 64 && ((uint64_t)1 << k) < n; k++) {
    const uint64_t step = (uint64_t)1 << k, m = std::min(step, n - step);
    for (uint64_t i = 0; i < m; i++) h_mul(f, out + (i + step) * L, out + i * L, hi + (size_t)k * L);
    if (lo)
      for (uint64_t i = 0; i < step; i++) h_mul(f, out + i * L, out + i * L, lo + (size_t)k * L);
  }
}

// K10 for both tensors (either may be null) on st; tab: room for n_points * tab_bits pairs
int tensors_enqueue(ErrText* err, const lcpc_ctx* c, uint32_t basis, const Shape& s, const uint32_t* d_points, uint32_t n_point,
                    uint32_t n_points, uint64_t n_rows, uint64_t n_per_row, uint32_t* d_tab, uint32_t* d_outer, uint32_t* d_inner,
                    hipStream_t st) {
  const uint32_t* one = reinterpret_cast<const uint32_t*>(c->f->r);
  hipError_t e = launch_eval_pairs(c->NL, (int)basis, d_points, n_point, n_points, s.tab_bits, one, d_tab, st);
  if (e != hipSuccess) return fail_hip(err, e, "launch_eval_pairs");
  if (d_inner) {
    e = launch_eval_expand(c->NL, (int)basis, d_tab, s.tab_bits, s.in_bits, n_per_row, 1, n_points, one, d_inner, st);
    if (e != hipSuccess) return fail_hip(err, e, "launch_eval_expand (inner)");
  }
  if (d_outer) {
    e = launch_eval_expand(c->NL, (int)basis, d_tab + (size_t)s.out_first * 2 * c->NL, s.tab_bits, s.out_bits, n_rows, s.out_stride, n_points,
                           one, d_outer, st);
    if (e != hipSuccess) return fail_hip(err, e, "launch_eval_expand (outer)");
  }
  return 0;
}

// Scratch of an evaluation, every segment a multiple of 256 bytes:
//   [points | evals (host entry only)] [pair table] [outer] [inner] (from points only) [polys] [K11's chunk sums] ... [collapse partials at the end]
struct EvalLayout {
  size_t pts = 0, evals = 0, tab = 0, outer = 0, inner = 0, polys = 0, parts = 0, total = 0;
};
EvalLayout eval_layout(const lcpc_commit_t* m, const Shape* s, uint32_t n_point, uint32_t n_points, bool host) {
  const lcpc_ctx* c = m->enc;
  const size_t eb = elem_bytes(c);
  EvalLayout l;
  size_t off = 0;
  auto seg = [&](size_t bytes) { const size_t at = off; off += up256(bytes ? bytes : 1); return at; };
  if (host) { l.pts = seg((size_t)n_points * n_point * eb); l.evals = seg((size_t)n_points * eb); }
  if (s) {
    l.tab = seg((size_t)n_points * s->tab_bits * 2 * eb);
    l.outer = seg((size_t)n_points * m->n_rows_local * eb);
    l.inner = seg((size_t)n_points * c->n_per_row * eb);
  }
  l.polys = seg((size_t)n_points * c->n_per_row * eb);
  l.parts = seg((size_t)field_dot_chunks(c->n_per_row, n_points) * n_points * eb);
  l.total = off + collapse_scratch_bytes(m, 2) + 512;       // collapse_range puts its partials at the end of the allocation
  return l;
}

// collapse with every outer tensor, dot with the matching inner tensor -> d_evals[n_points]; d_polys: room for [n_points][n_per_row],
// d_parts for K11's chunk sums
int eval_tensors_enqueue(lcpc_commit_t* m, DevScratch* sc, const uint32_t* d_outer, const uint32_t* d_inner, uint32_t n_points,
                         uint32_t* d_polys, uint32_t* d_parts, hipStream_t st, uint32_t* d_evals) {
  const lcpc_ctx* c = m->enc;
  int rc = collapse_run(m, sc, d_outer, n_points, st, d_polys);
  if (rc) return rc;
  HIPCHK(m, launch_field_dot(c->NL, d_polys, c->n_per_row, d_inner, c->n_per_row, c->n_per_row, n_points, d_evals, d_parts, st));
  return 0;
}

// the context's evaluation scratch (c->mu held) for work about to be enqueued on st: st waits for the kernel that last used it,
// the caller records c->ev_eval behind its own
int eval_scratch(lcpc_ctx* c, uint64_t bytes, hipStream_t st) {
  if (!c->ev_eval) HIPCHK(c, hipEventCreateWithFlags(&c->ev_eval, hipEventDisableTiming));
  else HIPCHK(c, hipStreamWaitEvent(st, c->ev_eval, 0));
  return ensure_dev(&c->err, &c->d_eval_tab, &c->eval_tab_cap, bytes + 16);
}

inline uint32_t* at(const DevScratch* sc, size_t off) { return reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(sc->d) + off); }

}  // namespace

extern "C" {

int lcpce_version(void) { return LCPCE_VERSION; }

int lcpce_tensors(uint32_t field, uint32_t basis, const uint64_t* point, uint32_t n_point, uint64_t n_rows, uint64_t n_per_row,
                  uint64_t* outer, uint64_t* inner) {
  const FieldDesc* fp = field_desc((int)field);
  Shape s;
  if (!fp || (!outer && !inner) || shape_of(basis, n_point, n_rows, n_per_row, &s)) return LCPC_ERR_ARG;
  if (n_point && !point) return LCPC_ERR_ARG;
  const FieldDesc& f = *fp;
  if (!all_reduced(f, point, n_point)) return LCPC_ERR_ARG;
  const int L = f.L;
  uint64_t hi[64 * MAXL], lo[64 * MAXL];
  const bool lagrange = basis == LCPCE_ML_LAGRANGE;
  if (basis != LCPCE_POWERS) {
    for (uint32_t k = 0; k < n_point; k++) {
      memcpy(hi + (size_t)k * L, point + (size_t)k * L, 8 * L);
      if (lagrange) h_sub(f, lo + (size_t)k * L, f.r, point + (size_t)k * L);
    }
    if (inner) expand_host(f, hi, lagrange ? lo : nullptr, n_per_row, inner);
    if (outer) expand_host(f, hi + (size_t)s.out_first * L, lagrange ? lo + (size_t)s.out_first * L : nullptr, n_rows, outer);
    return 0;
  }
  // hi[k] = x^(2^k); y = x^n_per_row from the bits of n_per_row; then the same chain from y for the rows
  auto squarings = [&](const uint64_t* from, unsigned n) {
    if (n) memcpy(hi, from, 8 * L);
    for (unsigned k = 1; k < n; k++) h_mul(f, hi + (size_t)k * L, hi + (size_t)(k - 1) * L, hi + (size_t)(k - 1) * L);
  };
  const unsigned nb = bit_len(n_per_row);
  squarings(point, nb);
  uint64_t y[MAXL];
  memcpy(y, f.r, 8 * L);
  for (unsigned k = 0; k < nb; k++)
    if ((n_per_row >> k) & 1) h_mul(f, y, y, hi + (size_t)k * L);
  if (inner) expand_host(f, hi, nullptr, n_per_row, inner);
  if (outer) {
    squarings(y, bit_len(n_rows - 1));
    expand_host(f, hi, nullptr, n_rows, outer);
  }
  return 0;
}

int lcpce_tensors_device(lcpc_ctx* c, uint32_t basis, const uint64_t* points_dev, uint32_t n_point, uint32_t n_points, uint64_t n_rows,
                         uint64_t n_per_row, uint64_t* outer_dev, uint64_t* inner_dev, void* stream) {
  Shape s;
  if (!c || (!outer_dev && !inner_dev) || n_points == 0 || n_points > MAX_POINTS) return LCPC_ERR_ARG;
  if (shape_of(basis, n_point, n_rows, n_per_row, &s) || (n_point && !points_dev)) return LCPC_ERR_ARG;
  if (!dev_aligned(points_dev, c->L) || !dev_aligned(outer_dev, c->L) || !dev_aligned(inner_dev, c->L)) return LCPC_ERR_ARG;
  if ((n_rows + 255) / 256 > 0x7fffffffu || (n_per_row + 255) / 256 > 0x7fffffffu) return LCPC_ERR_ARG;      // the expansion's grid
  LCPC_TRY
  hipStream_t st = (hipStream_t)stream;
  std::lock_guard<std::mutex> g(c->mu);
  HIPCHK(c, hipSetDevice(c->prm.device));
  int rc = eval_scratch(c, (uint64_t)n_points * s.tab_bits * 2 * elem_bytes(c), st);
  if (rc) return rc;
  rc = tensors_enqueue(&c->err, c, basis, s, reinterpret_cast<const uint32_t*>(points_dev), n_point, n_points, n_rows, n_per_row,
                       c->d_eval_tab, reinterpret_cast<uint32_t*>(outer_dev), reinterpret_cast<uint32_t*>(inner_dev), st);
  if (rc) return rc;
  HIPCHK(c, hipEventRecord(c->ev_eval, st));
  return 0;
  LCPC_CATCH(c)
}

int lcpce_dot_device(lcpc_ctx* c, const uint64_t* a_dev, uint64_t a_stride, const uint64_t* b_dev, uint64_t b_stride, uint64_t n,
                     uint32_t n_pairs, uint64_t* out_dev, void* stream) {
  if (!c || !a_dev || !b_dev || !out_dev || n == 0 || n_pairs == 0 || n_pairs > MAX_POINTS) return LCPC_ERR_ARG;
  if (!dev_aligned(a_dev, c->L) || !dev_aligned(b_dev, c->L) || !dev_aligned(out_dev, c->L)) return LCPC_ERR_ARG;
  LCPC_TRY
  hipStream_t st = (hipStream_t)stream;
  const uint32_t n_chunks = field_dot_chunks(n, n_pairs);
  std::unique_lock<std::mutex> g(c->mu, std::defer_lock);
  HIPCHK(c, hipSetDevice(c->prm.device));
  uint32_t* parts = nullptr;
  if (n_chunks > 1) {                       // the chunk sums live in the context's evaluation scratch: as lcpce_tensors_device
    g.lock();
    int rc = eval_scratch(c, (uint64_t)n_chunks * n_pairs * elem_bytes(c), st);
    if (rc) return rc;
    parts = c->d_eval_tab;
  }
  HIPCHK(c, launch_field_dot(c->NL, reinterpret_cast<const uint32_t*>(a_dev), a_stride, reinterpret_cast<const uint32_t*>(b_dev), b_stride, n,
                             n_pairs, reinterpret_cast<uint32_t*>(out_dev), parts, st));
  if (parts) HIPCHK(c, hipEventRecord(c->ev_eval, st));
  return 0;
  LCPC_CATCH(c)
}

int lcpce_eval_tensors_device(lcpc_commit_t* m, const uint64_t* outer_dev, const uint64_t* inner_dev, uint32_t n_points, void* stream,
                              uint64_t* evals_dev) {
  if (!m || !outer_dev || !inner_dev || !evals_dev || n_points == 0 || n_points > MAX_POINTS) return LCPC_ERR_ARG;
  const lcpc_ctx* c = m->enc;
  if (!dev_aligned(outer_dev, c->L) || !dev_aligned(inner_dev, c->L) || !dev_aligned(evals_dev, c->L)) return LCPC_ERR_ARG;
  if (c->prm.shard_count > 1) return LCPC_ERR_STATE;
  LCPC_TRY
  std::shared_lock<FillLock> rd(m->fill_mu);
  if (!m->committed) return LCPC_ERR_STATE;
  std::lock_guard<std::mutex> g(m->mu);
  HIPCHK(m, hipSetDevice(c->prm.device));
  const EvalLayout l = eval_layout(m, nullptr, 0, n_points, false);
  int rc = ensure_scratch(m, &m->sc, l.total);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = order_after_commit(m, st))) return rc;
  return eval_tensors_enqueue(m, &m->sc, reinterpret_cast<const uint32_t*>(outer_dev), reinterpret_cast<const uint32_t*>(inner_dev), n_points,
                              at(&m->sc, l.polys), at(&m->sc, l.parts), st, reinterpret_cast<uint32_t*>(evals_dev));
  LCPC_CATCH(m)
}

int lcpce_eval_device(lcpc_commit_t* m, uint32_t basis, const uint64_t* points_dev, uint32_t n_point, uint32_t n_points, void* stream,
                      uint64_t* evals_dev) {
  if (!m || !evals_dev || basis > LCPCE_ML_LAGRANGE || n_points == 0 || n_points > MAX_POINTS || (n_point && !points_dev)) return LCPC_ERR_ARG;
  const lcpc_ctx* c = m->enc;
  if (!dev_aligned(points_dev, c->L) || !dev_aligned(evals_dev, c->L)) return LCPC_ERR_ARG;
  if (c->prm.shard_count > 1) return LCPC_ERR_STATE;
  LCPC_TRY
  std::shared_lock<FillLock> rd(m->fill_mu);
  if (!m->committed) return LCPC_ERR_STATE;
  Shape s;
  if (shape_of(basis, n_point, m->n_rows, c->n_per_row, &s)) return LCPC_ERR_ARG;
  std::lock_guard<std::mutex> g(m->mu);
  HIPCHK(m, hipSetDevice(c->prm.device));
  const EvalLayout l = eval_layout(m, &s, n_point, n_points, false);
  int rc = ensure_scratch(m, &m->sc, l.total);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = order_after_commit(m, st))) return rc;
  DevScratch* sc = &m->sc;
  if ((rc = tensors_enqueue(&m->err, c, basis, s, reinterpret_cast<const uint32_t*>(points_dev), n_point, n_points, m->n_rows, c->n_per_row,
                            at(sc, l.tab), at(sc, l.outer), at(sc, l.inner), st)))
    return rc;
  return eval_tensors_enqueue(m, sc, at(sc, l.outer), at(sc, l.inner), n_points, at(sc, l.polys), at(sc, l.parts), st, reinterpret_cast<uint32_t*>(evals_dev));
  LCPC_CATCH(m)
}

int lcpce_eval(lcpc_commit_t* m, uint32_t basis, const uint64_t* points_host, uint32_t n_point, uint32_t n_points, uint64_t* evals_host) {
  if (!m || !evals_host || basis > LCPCE_ML_LAGRANGE || n_points == 0 || n_points > MAX_POINTS || (n_point && !points_host)) return LCPC_ERR_ARG;
  const lcpc_ctx* c = m->enc;
  if (c->prm.shard_count > 1) return LCPC_ERR_STATE;
  LCPC_TRY
  std::shared_lock<FillLock> rd(m->fill_mu);
  if (!m->committed) return LCPC_ERR_STATE;
  Shape s;
  if (shape_of(basis, n_point, m->n_rows, c->n_per_row, &s)) return LCPC_ERR_ARG;
  if (!all_reduced(*c->f, points_host, (uint64_t)n_points * n_point)) return LCPC_ERR_ARG;
  SetLease<CallSet> lease{m->sets};
  int rc = take_call_set(m, 0, &lease.s);
  if (rc) return rc;
  CallSet* ws = lease.s;
  const EvalLayout l = eval_layout(m, &s, n_point, n_points, true);
  if ((rc = ensure_scratch(m, &ws->sc, l.total))) return rc;
  DevScratch* sc = &ws->sc;
  hipStream_t st = ws->st;
  const size_t eb = elem_bytes(c);
  if (n_point) HIPCHK(m, hipMemcpyAsync(at(sc, l.pts), points_host, (size_t)n_points * n_point * eb, hipMemcpyHostToDevice, st));
  if ((rc = tensors_enqueue(&m->err, c, basis, s, at(sc, l.pts), n_point, n_points, m->n_rows, c->n_per_row, at(sc, l.tab), at(sc, l.outer),
                            at(sc, l.inner), st)))
    return rc;
  if ((rc = eval_tensors_enqueue(m, sc, at(sc, l.outer), at(sc, l.inner), n_points, at(sc, l.polys), at(sc, l.parts), st, at(sc, l.evals)))) return rc;
  HIPCHK(m, hipMemcpyAsync(evals_host, at(sc, l.evals), (size_t)n_points * eb, hipMemcpyDeviceToHost, st));
  HIPCHK(m, hipStreamSynchronize(st));
  return 0;
  LCPC_CATCH(m)
}

}  // extern "C"
