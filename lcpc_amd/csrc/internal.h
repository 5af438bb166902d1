// lcpc_amd/csrc/internal.h -- shared internals of the C ABI implementation (include/lcpc_hip.h).
//
//   ctx.cpp     lcpc_ctx     = an LcEncoding implementor (ligero lib.rs:31-186, brakedown lib.rs:41-176): twiddle tables /
//                              expander matrices on the device, dims, batched encode.  Immutable after creation, shared
//                              by any number of commitments (the reference's `&E`, lcpc-2d lib.rs:74-104).
//   commit.cpp  lcpc_commit  = an LcCommit<D, E> (lcpc-2d lib.rs:172-184): comm / coeffs / hashes in HBM, created by
//                              commit(), consumed by prove / open_column / collapse_columns.
//   prove.cpp   transcript wrappers, prove (lib.rs:1004-1093), verify (lib.rs:832-1000), bincode (lib.rs:550-609)
//   verify_batch.cpp  lcpcv_verify_batch (include/lcpc_hip_verify.h): the verifier's batch call over K7b
//   shard.cpp   row-sharded commit / prove across GPUs and the RCCL exchange
#pragma once
#include "../../include/lcpc_hip.h"
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>
#include "encoding.h"
#include "host_crypto.h"
#include "host_field.h"
#include "host_par.h"
#include "kernels.h"

namespace lcpc {

struct DevCsr {
  uint64_t n_in = 0, n_out = 0;
  uint32_t *rowptr = nullptr, *colidx = nullptr, *vals = nullptr;
  uint32_t* vals29 = nullptr;     // Ft255: values in the 29-bit-limb / 2^261 form (ln::lazy_mac)
};
// one pass of the Ligero row NTT as the context plans it (ctx.cpp plan_passes, build_limb_plan): everything about the pass that
// does not depend on the job.  A step with a.log_n < the context's log_n runs on n_rows << (log_n - a.log_n) sub-rows.
struct NttStep {
  enum Kernel { GENERAL, K1S, K1N } kernel = GENERAL;   // kernels.hip launch_ntt_pass / ntt_l9s.hip (Ft255) / ntt_lns.hip
  bool first = false;              // K1s / K1n: the first-pass kernel
  int log_tile = 0;                // general kernel
  NttPassArgs a{};                 // log_n, t0, s, log_tj of the (sub-)transform; the tables (roots, roots29, qp29, wq_w); tile_group,
                                   // canon_row_mask
  const uint32_t* roots29c = nullptr;   // canonical output only: the converting table, and what the pass leaves to convert
  uint32_t mont_prefix = 0, blk0_gone = 0;
  uint32_t* pack = nullptr;        // K1s / K1n: the lane-order twiddle pack (owned by the context)
  NttPackInfo pack_info{};
};

// device working buffers of one Brakedown encode: owned by a commitment (where the position-major copy IS the
// commitment matrix) or, for lcpc_encode_rows, by the encoder context
struct EncodeWs {
  uint32_t* d_tmp = nullptr;       // last precode output, n_rows x m_last
  uint64_t tmp_cap = 0;            // bytes
  uint32_t* d_t = nullptr;         // position-major working copy T[pos][row] of the rows being encoded
  uint64_t t_cap = 0;              // bytes
  uint32_t* d_mid = nullptr;       // Ligero, Ft255 two-pass plans: the 29-bit-limb intermediate between the passes (ntt_l9s.hip),
  uint64_t mid_cap = 0;            // rows_per_batch x n_cols x 36 bytes (bytes)
  bool mid_failed = false;         // the allocation failed once: stay on the packed intermediate (comm itself)
};
// rows whose limb intermediate fits LCPC_NTT_MID_MAX_MB (default 6144 MiB: the whole headline commitment in one batch; 0 = off)
uint64_t ntt_mid_rows(const lcpc_ctx* c, uint64_t n_rows);

// Brakedown: from this many rows on the rows are encoded on a position-major copy (lane = row); below, row-major with
// lanes over outputs and terms
constexpr uint64_t SDIG_T_MIN_ROWS = 24;

// proof buffers (prove.cpp): lcpc_free hands them back; one is kept for the next proof
void* proof_buf_alloc(size_t n);
void proof_buf_free(void* p);

// The detail text of an object's last failure (lcpc_last_error, lcpc_commit_last_error).  Calls on one object may fail on several
// threads at once, so a failure writes its text under a lock of its own into the next of four fixed buffers and then publishes
// that buffer: the pointer a getter returned stays valid for the object's lifetime, and after concurrent failures the text is
// that of one of them.  (Its own lock, not the object's `mu`: a failure is often reported from inside a `mu` section.)
class ErrText {
 public:
  ErrText& operator=(const std::string& s) { set(s.c_str()); return *this; }
  ErrText& operator=(const char* s) { set(s); return *this; }
  void clear() { set(""); }
  const char* c_str() const { return buf_[cur_.load(std::memory_order_acquire)]; }
 private:
  void set(const char* s) {
    std::lock_guard<std::mutex> g(mu_);
    const unsigned k = (cur_.load(std::memory_order_relaxed) + 1) % 4;
    snprintf(buf_[k], sizeof buf_[k], "%s", s ? s : "");
    cur_.store(k, std::memory_order_release);
  }
  std::mutex mu_;
  std::atomic<unsigned> cur_{0};
  char buf_[4][512] = {};
};

// The shared / exclusive lock of a commitment's contents (lcpc_commit_s::fill_mu).  A waiting fill goes before readers that
// arrive after it: glibc's std::shared_mutex prefers readers, and a loop of proves on one thread could hold a refill off for good.
// Not recursive in either mode (a reader that re-locked behind a waiting fill would deadlock): the entry points lock, internals don't.
class FillLock {
 public:
  void lock() {
    std::unique_lock<std::mutex> g(mu_);
    ++fills_waiting_;
    cv_.wait(g, [&] { return !filling_ && readers_ == 0; });
    --fills_waiting_;
    filling_ = true;
  }
  void unlock() {
    { std::lock_guard<std::mutex> g(mu_); filling_ = false; }
    cv_.notify_all();
  }
  void lock_shared() {
    std::unique_lock<std::mutex> g(mu_);
    cv_.wait(g, [&] { return !filling_ && fills_waiting_ == 0; });
    ++readers_;
  }
  void unlock_shared() {
    bool last;
    { std::lock_guard<std::mutex> g(mu_); last = --readers_ == 0; }
    if (last) cv_.notify_all();
  }
 private:
  std::mutex mu_;
  std::condition_variable cv_;
  unsigned readers_ = 0, fills_waiting_ = 0;
  bool filling_ = false;
};

// device scratch of collapse / open: the working buffers of one call at a time (a commitment's own, or a working set's)
struct DevScratch {
  uint32_t* d = nullptr;           // [tensors][polys][canonical polys] ... [collapse partials at the end]; open: [cols][vals][paths]
  uint64_t cap = 0;                // bytes
  uint32_t* t29 = nullptr;         // collapse: tensors in the 29-bit-limb form
  uint64_t t29_cap = 0;
  void release() { if (d) (void)hipFree(d); if (t29) (void)hipFree(t29); d = t29 = nullptr; cap = t29_cap = 0; }
};

// What one prove / collapse / open call on a commitment works in, so that calls on one commitment run side by side: its own
// non-blocking stream (ordered behind the commit that filled the object when the set is taken), the slice events of prove's
// collapse, device scratch, and prove's pinned arena (tensors, polynomials, their canonical forms).
struct CallSet {
  bool busy = false;
  uint8_t* h_pin = nullptr;
  uint64_t h_pin_cap = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev_slice[2] = {nullptr, nullptr};   // arrival of the two column ranges of p_random on the host (collapse_host_sliced)
  DevScratch sc;
  int make();                      // stream and events (on the current device)
  void quiesce() { (void)hipStreamSynchronize(st); }   // (a call that failed half-way may have left work on the stream)
  ~CallSet();
};
// lcpc_verify's host working set (encoded rows as they come back, to_repr of the polynomials): pinned, kept between calls
// (a fresh 150 MB of pageable memory costs ~20 ms in first-touch faults and munmap at Brakedown 2^27)
struct VerifySet {
  bool busy = false;
  uint8_t* h_pin = nullptr;
  uint64_t h_pin_cap = 0;
  int make() { return 0; }
  void quiesce() {}
  ~VerifySet() { if (h_pin) (void)hipHostFree(h_pin); }
};

// lcpcv_verify_batch's working set (verify_batch.cpp): its own non-blocking stream, the event behind the row encode, the pinned arena of
// a group and the device buffers of a group.  Batch verifies under one encoder run side by side, each in its own.
struct VerifyBatchSet {
  bool busy = false;
  uint8_t* h_pin = nullptr;
  uint64_t h_pin_cap = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev_enc = nullptr;     // recorded behind the row encode: the encoder's lock is held until it has fired
  uint8_t* d = nullptr;            // [polys][encoded rows][columns][canonical columns][tensors][drawn][status][digests (+ CVs)]
  uint64_t d_cap = 0;
  uint32_t* t29 = nullptr;         // Ft255: the tensors in the 29-bit-limb form
  uint64_t t29_cap = 0;
  // the Merkle path siblings the device folds (K8b): a pinned buffer and its device mirror, beside the arena and not part of its
  // formula; grown on demand (ensure_paths)
  uint8_t* h_path = nullptr;
  uint8_t* d_path = nullptr;
  uint64_t h_path_cap = 0, d_path_cap = 0;
  int make();
  int ensure_paths(ErrText* err, uint64_t bytes);
  void quiesce() { (void)hipStreamSynchronize(st); }
  ~VerifyBatchSet();
};

// Working sets of concurrent calls on one object.  A call takes a set on entry (take) and hands it back on exit (SetLease).
// Sets are made on first need and kept with the object, at most MAX_SETS of them: a caller beyond that waits for a set to come
// back.  take() also sizes the set's pinned arena; when that allocation fails while the object has another set whose arena is
// large enough, the caller waits for that one instead of failing.  `mu` guards only this bookkeeping.
template <typename S> class SetPool {
 public:
  static constexpr size_t MAX_SETS = 8;
  // the device of the object must be current (a new set's stream is made on it); 0, LCPC_ERR_NOMEM or a HIP error code
  int take(uint64_t pin_bytes, S** out) {
    *out = nullptr;
    std::unique_lock<std::mutex> lk(mu_);
    bool reuse_only = false;       // a pinned allocation failed: only a set that already holds pin_bytes will do
    for (;;) {
      S* pick = nullptr;
      for (auto& s : sets_) if (!s->busy && s->h_pin_cap >= pin_bytes) { pick = s.get(); break; }
      if (!pick && !reuse_only) {
        for (auto& s : sets_) if (!s->busy) { pick = s.get(); break; }
        if (!pick && sets_.size() < MAX_SETS) {
          std::unique_ptr<S> s(new S());
          if (int rc = s->make()) return rc;
          sets_.push_back(std::move(s));
          pick = sets_.back().get();
        }
      }
      if (!pick) {
        if (reuse_only && !any_holds(pin_bytes)) return LCPC_ERR_NOMEM;
        cv_.wait(lk);
        continue;
      }
      pick->busy = true;
      if (pick->h_pin_cap >= pin_bytes) { *out = pick; return 0; }
      lk.unlock();                 // (the set is this caller's: pinning runs outside the bookkeeping lock)
      if (pick->h_pin) (void)hipHostFree(pick->h_pin);
      pick->h_pin = nullptr; pick->h_pin_cap = 0;
      void* hp = nullptr;
      const bool ok = hipHostMalloc(&hp, (size_t)pin_bytes, hipHostMallocDefault) == hipSuccess;
      if (!ok) (void)hipGetLastError();
      lk.lock();
      if (ok) { pick->h_pin = static_cast<uint8_t*>(hp); pick->h_pin_cap = pin_bytes; *out = pick; return 0; }
      pick->busy = false;
      if (!any_holds(pin_bytes)) return LCPC_ERR_NOMEM;
      reuse_only = true;
    }
  }
  void give(S* s) {
    { std::lock_guard<std::mutex> g(mu_); s->busy = false; }
    cv_.notify_all();
  }
  void clear() { sets_.clear(); }  // (destroy: no call is running)
 private:
  bool any_holds(uint64_t pin_bytes) const {
    for (auto& s : sets_) if (s->h_pin_cap >= pin_bytes) return true;
    return false;
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<std::unique_ptr<S>> sets_;
};
// a taken set, handed back on every exit path -- with nothing of its call left in flight
template <typename S> struct SetLease {
  SetPool<S>& pool;
  S* s = nullptr;
  ~SetLease() { if (s) { s->quiesce(); pool.give(s); } }
};

// The storage of one batched commit (batch.cpp, include/lcpc_hip_batch.h): comm, coeffs, hashes and the chunk chaining values of
// every member in ONE device allocation, member-major, so that the row encode sees one matrix of n_batch * n_rows rows and the batched
// hash / tree kernels reach member i at a fixed stride.  The members share it (lcpc_commit_s::slab); the last one to leave frees it.
// A hashes slot is digest_words(c) words (8; BLAKE2b 16); only BLAKE3 has chunk chaining values.
// Two regimes: a slab with a `comm` segment (Ligero; Brakedown members of < SDIG_T_MIN_ROWS rows) holds row-major commitment
// matrices, and a member's d_comm / d_coeffs / d_hashes are views into it.  A slab with a `t` segment instead (Brakedown members
// of >= SDIG_T_MIN_ROWS rows) holds every member's position-major T[pos][row]: the member's ws.d_t is the view (comm_t), and its
// d_comm is null or the member's OWN row-major copy made on demand (lcpc_get_comm).  leave_slab before anything frees or regrows
// a view.
struct BatchSlab {
  uint8_t* d = nullptr;
  uint64_t off_comm = 0, off_t = 0, off_coeffs = 0, off_hashes = 0, off_cvs = 0;   // bytes; a segment is member-major
  uint64_t comm_stride = 0, t_stride = 0, coeffs_stride = 0, hashes_stride = 0, cvs_stride = 0;   // 32-bit words per member (0: no such segment)
  uint64_t tmp_stride = 0;         // t regime: words per member of ws.d_tmp (the last precode's [o][row] of every member)
  uint32_t n_batch = 0;
  uint64_t n_rows = 0;
  uint32_t* h_roots = nullptr;     // pinned, device-mapped [n_batch][digest_words]: written by the launch that produces the roots
  uint32_t* d_roots_alias = nullptr;
  EncodeWs ws;                     // the batch's row encode (a batch call holds every member's lock)
  uint32_t* seg(uint64_t off, uint64_t stride, uint32_t i) const { return reinterpret_cast<uint32_t*>(d + off) + (size_t)i * stride; }
  ~BatchSlab() {
    if (d) (void)hipFree(d);
    if (ws.d_tmp) (void)hipFree(ws.d_tmp);
    if (ws.d_t) (void)hipFree(ws.d_t);
    if (ws.d_mid) (void)hipFree(ws.d_mid);
    if (h_roots) (void)hipHostFree(h_roots);
  }
};

}  // namespace lcpc

struct lcpc_transcript {
  lcpc::Transcript t;
  lcpc_transcript(const uint8_t* l, size_t n) : t(l, n) {}
};

namespace lcpc {
// a cached two-level table on the device (fft.cpp cached_table): the twiddles of a size and direction (kernels.h launch_fft), or the
// powers of a shift (launch_coset_fft), whose key has the shift's limbs as well -- a twiddle table's are all zero, which no shift is
struct FftTab {
  uint64_t shift[4] = {0, 0, 0, 0};
  uint32_t log_n = 0;
  bool inverse = false;
  uint32_t* d = nullptr;           // fft_tab_elems(log_n) elements
  uint64_t stamp = 0;              // last use
};
}  // namespace lcpc

struct lcpc_ctx {
  lcpc_params prm{};
  // A/B switches, read from the environment ONCE, when the context is created (never on a launch path: getenv next to a
  // setenv of another thread is undefined behaviour, and a context must not change plans under a running commit)
  bool sw_ntt_general = false;     // LCPC_NTT_GENERAL: every Ligero row on the general kernel (K1) instead of the shape-specialised plans
  int sw_ntt_mul = -1;             // LCPC_NTT_MUL=mont|split: the lane-varying multiplier of the K1s pure / coset plans (ntt_l9s.hip M2): 0 = ln::mul,
                                   // 1 = ln::mul2 on split packs in every pass that has the instantiation, 2 / 3 (split-pure / split-coset) = in that pass alone,
                                   // -1 (unset) = per pass (build_limb_plan)
  int sw_ntt_form = -1;            // LCPC_NTT_FORM=dif|coset: the K1s two-pass plans' factorisation (ntt_l9s.hip): 0 = DIF, 1 = pure first pass + coset
                                   // last pass at every size, -1 (unset) = coset from 2^16 columns on (build_limb_plan)
  int64_t sw_ntt_mid_max_mb = -1;  // LCPC_NTT_MID_MAX_MB: -1 = the default rule of ntt_mid_rows
  bool sw_debug_timing = false;    // LCPC_DEBUG_TIMING: phase times of construction / prove / verify on stderr
  // forced allocation failures: set and read only in lib/liblcpc_hip_testhooks.so (the tests' second build of ctx.cpp, with
  // LCPC_TEST_HOOKS); members in every build, so that all objects of that library see one layout of the struct
  bool sw_test_fail_3pass = false; // LCPC_TEST_FAIL=3pass: the three-pass plan's tables "do not fit" -> the general kernel's plan
  bool sw_test_fail_mid = false;   // LCPC_TEST_FAIL=mid: the K1s limb-intermediate allocation fails -> packed intermediate
  const lcpc::FieldDesc* f = nullptr;
  int L = 0, NL = 0;
  uint64_t n_per_row = 0, n_cols = 0, np2 = 0;
  uint32_t path_len = 0;
  // Ligero
  unsigned log_n = 0;
  uint32_t* d_roots = nullptr;
  // lazy-limb NTT tables, N limbs of W bits per entry, `stride` words (ntt_lns_limbs / _limb_bits / _stride; field_ln.h LnField):
  // Ft255's (9, 29, 12) are made with d_roots and read by the general kernel as well (ntt_pass_l9_kernel); those of Ft63 / Ft127 /
  // Ft191 are made only for a K1n plan
  uint32_t* d_rootsl = nullptr;    // w^i R' mod p (Ft255: R' = 2^261, field_ln.h fe_mul_r29; R' = 2^(N W))
  uint32_t* d_rootslc = nullptr;   // w^i R' R^-1 mod p (Ft255: w^i 2^5): the table that converts to canonical on the fly
  uint32_t* d_qpl = nullptr;       // (i - 24) * p, i < 64, same form (ln::clamp, ln::clamp_*)
  uint32_t* d_rootsls = nullptr;   // three-pass plans: the 2^20-point tables (every 2^(log_n - 20)-th entry of d_rootsl / d_rootslc)
  uint32_t* d_rootslcs = nullptr;
  uint32_t* d_wq_w = nullptr;      // the shifted multiples of the primitive 4th root w^(n/4) (the same element for every n), 96 words
  // the row NTT: the general kernel's passes (K1, plan_passes), or a lazy-limb plan (build_limb_plan) -- two passes on 1024-element
  // tiles, or for 2^21 .. 2^26 columns three: a first pass over the whole rows, then the 2^20-point two-pass plan per block
  std::vector<lcpc::NttStep> ntt;
  bool comm_canon = false;         // d_comm of a commit holds canonical values (x * R^-1), not Montgomery form: the column
                                   // hash reads them as they are; every read-out (get_comm, open_columns) converts back
                                   // (Brakedown: the position-major commitment of a commit -- ws.d_t, >= SDIG_T_MIN_ROWS rows -- always holds
                                   // canonical values: converted once in the input transpose, kept by every (linear) level)
  // Brakedown
  lcpc::SdigSpec spec{};
  std::vector<lcpc::LevelDims> pre_dims, post_dims;
  std::vector<lcpc::DevCsr> d_pre, d_post;
  uint32_t* d_r2 = nullptr;
  // lcpc_encode_rows (the verifier's row encodes): scratch under `mu`
  lcpc::EncodeWs ws;
  uint32_t* d_scratch = nullptr;
  uint64_t scratch_cap = 0;
  // lcpce_tensors_device / lcpce_dot_device (include/lcpc_hip_eval.h): the pair table of K10 or the chunk sums of K11, under `mu`.
  // The calls only enqueue, on the caller's stream: ev_eval is recorded behind the kernel that last used the buffer, and the next
  // call's stream waits for it
  uint32_t* d_eval_tab = nullptr;
  uint64_t eval_tab_cap = 0;
  hipEvent_t ev_eval = nullptr;
  // lcpcf_fft_device / lcpcf_commit_evals* (include/lcpc_hip_fft.h): the two-level twiddle tables of the last few (size, direction)
  // pairs, under `mu`; made on first use (fft.cpp fft_enqueue), read-only afterwards, so streams need no order among each other --
  // an evicted table is freed by hipFree, which waits for the kernels that still read it
  lcpc::FftTab fft_tabs[4];
  uint64_t fft_stamp = 0;
  // the lcpcd_ device calls (include/lcpc_hip_domain.h): the shift tables of the last few (shift, size, direction) keys, under `mu`,
  // by the same routine (domain.cpp dom_table); they share fft_stamp
  lcpc::FftTab dom_tabs[8];
  // RCCL communicator of a sharded encoder (lcpc_comm_init); opaque ncclComm_t
  void* comm = nullptr;
  std::mutex xchg_mu;              // serialises the submission of collectives on `comm` (several commitments, several host threads)
  hipEvent_t ev_xchg = nullptr;    // recorded behind the last collective enqueued on `comm`; the next one's stream waits for it: the
                                   // collectives of one communicator run in submission order whatever streams they are enqueued on
                                   // (two commitments' exchange streams, a prove stream) -- under xchg_mu
  std::atomic<int> refs{1};        // the handle itself + one per live lcpc_commit
  lcpc::ErrText err;
  std::mutex mu;
  // lcpc_verify: one pinned host working set per running call (verifies under one encoder run side by side); the row encodes of a
  // verify run on s_verify under `mu` (ws / d_scratch above), which is held only around that encode's enqueue and synchronisation
  lcpc::SetPool<lcpc::VerifySet> verify_sets;
  hipStream_t s_verify = nullptr;  // non-blocking
  // lcpcv_verify_batch (include/lcpc_hip_verify.h): one working set per running call; its row encode runs on the set's stream under
  // `mu` (ws above), which is held until that encode's event has fired
  lcpc::SetPool<lcpc::VerifyBatchSet> verify_batch_sets;
  // lcpc_commit from PAGEABLE host memory (commit.cpp upload_host): a ring of pinned bounce buffers the host pool fills while
  // the previous slices cross the bus.  stage_mu is held per upload call (one row batch of one commit); the buffers are kept between commits
  // (up to 4 x 64 MiB of pinned host memory per encoder that has taken a pageable source; LCPC_HOST_STAGE=1 pins the first two at lcpc_ctx_create).
  std::mutex stage_mu;
  static constexpr unsigned N_STAGE = 4;
  uint8_t* h_stage[N_STAGE] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_stage[N_STAGE] = {nullptr, nullptr, nullptr, nullptr};   // the H2D copy that last read h_stage[k]
  size_t stage_cap = 0;            // bytes per buffer
  unsigned stage_next = 0;
  int32_t sw_host_stage = -1;      // LCPC_HOST_STAGE: 0 = never stage (the runtime's own pageable path), 1 = always stage, -1 (unset) = by pointer attributes
};

struct lcpc_commit_s {
  lcpc_ctx* enc = nullptr;
  bool committed = false;
  uint64_t n_rows = 0;             // rows of the whole commitment
  uint64_t row_begin = 0, n_rows_local = 0;
  uint64_t chunk_begin = 0, chunk_end = 0, n_chunks = 0;
  uint32_t *d_coeffs = nullptr, *d_comm = nullptr, *d_hashes = nullptr, *d_cvs = nullptr;
  const uint32_t* coeffs_view = nullptr;   // LcCommit.coeffs as prove/collapse read it: d_coeffs, or the caller's buffer
                                           // when the commit was made with LCPC_COMMIT_BORROW_COEFFS
  uint64_t cap_coeff_rows = 0, cap_comm_rows = 0, cap_cvs = 0;
  std::shared_ptr<lcpc::BatchSlab> slab;   // member of a batched commit: d_comm (or ws.d_t: BatchSlab) / d_coeffs / d_hashes are views into it,
  uint32_t slab_index = 0;                 // not allocations (leave_slab, commit.cpp)
  uint32_t* d_chain = nullptr;     // host-memory commit under SHA3-256 / Keccak-256 / SHA-256 / BLAKE2b: every column's chaining value between
  uint64_t cap_chain = 0;          // the row batches (kernels.h launch_chain_leaves_range), word-major; capacity in bytes; kept across refills
  lcpc::EncodeWs ws;
  bool comm_t = false;             // Brakedown commit with >= sdig_t_min_rows() local rows: the commitment matrix lives in ws.d_t (position-major,
                                   // element (row, col) at (col * n_rows_local + row)); hash / open read it there, d_comm is only
                                   // filled on demand (lcpc_get_comm) -- no back-transpose on the commit path
  bool comm_rows_valid = false;    // d_comm holds the row-major copy of the commitment in ws.d_t
  uint32_t* d_node_tab = nullptr;  // sharded finish: node_slot[0..n) then node_log[0..n) -- the current shape's entry of node_tabs
  uint64_t node_tab_key = 0;
  std::vector<uint32_t> node_slot_h, node_log_h;
  struct NodeTab { uint64_t key; uint32_t* d; std::vector<uint32_t> slot, lg; };
  std::vector<NodeTab> node_tabs;  // one device table per shape seen, freed with the object (never while a finish step may read it)
  uint8_t* d_gather = nullptr;     // native sharded commit (lcpc_commit_sharded_device): this rank's nodes + the all-gather output
  uint64_t gather_cap = 0;
  uint8_t *d_xsend = nullptr, *d_xrecv = nullptr;   // native sharded prove: exchange buffers
  uint64_t xchg_cap = 0;
  // scratch of the device-entry collapse (lcpc_collapse_device) and of the sharded prove; the host-entry prove / collapse / open
  // work in a set of `sets`
  lcpc::DevScratch sc;
  uint32_t* h_root = nullptr;      // pinned, device-mapped: the Merkle kernel that produces the root writes it here as well
  uint32_t* d_root_alias = nullptr;  // ... through this device address (null: no mapping, the root is copied out)
  // timing
  bool timing = false;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // start | encoded | hashed | done; [4]: the commit's stream
                                   // has the leaf digests (sharded commit: behind the exchange); [5]: the exchange's collectives are done
  hipStream_t s_prove = nullptr;   // sharded prove: its device steps and the native exchange, ordered behind the commit by ev_done
  hipEvent_t ev_done = nullptr;    // recorded behind every fill, on the stream that completed it (seal_commit): readers, refills and
                                   // the sharded prove's stream wait for it
  // native sharded commit (shard.cpp): the exchange stream of an async tail and its hand-over event
  hipStream_t s_xchg = nullptr;
  hipEvent_t ev_hashed = nullptr;  // recorded on the caller's stream behind the local column hash; s_xchg waits for it
  bool shard_encoded = false;      // split phases: the encode step of a sharded commit has been enqueued, hash / finish / merkle may follow
  hipStream_t s_copy = nullptr, s_comp = nullptr;   // lcpc_commit (host pointer): H2D of row batch b+1 overlaps the NTTs of batch b
  hipEvent_t ev_batch[16] = {nullptr};
  uint8_t* d_ints = nullptr;       // host commit from plain integers narrower than an element (lcpci_commit_ints): the integers as uploaded,
  uint64_t cap_ints = 0;           // widened from here into d_coeffs; capacity in bytes; kept across refills
  // Concurrency (include/lcpc_hip.h "Threads"): every fill (the commit entry points, from_parts, from_bincode) holds fill_mu
  // exclusively; every reader (prove, collapse, open, the getters) holds it shared for its whole duration.  A refill therefore waits
  // for the readers in flight, and no reader sees a half-filled object.  Lock order: fill_mu, then mu.
  mutable lcpc::FillLock fill_mu;
  lcpc::SetPool<lcpc::CallSet> sets;   // host-entry prove / collapse / open: one working set per running call
  std::mutex shard_prove_mu;       // held for a whole SHARDED prove: its collectives go out on one communicator, and every rank must
                                   // submit them in the same order -- two sharded proves of one commitment interleaving their
                                   // exchanges differently on two ranks would pair the wrong buffers (or hang)
  lcpc_timings last{};
  uint32_t launches[3] = {0, 0, 0};
  lcpc::ErrText err;
  std::mutex mu;                   // short sections: lazy allocation, the sharded and device-entry paths' scratch
};

namespace lcpc {

// ---- error plumbing ---------------------------------------------------------------------------------
inline int fail_hip(ErrText* err, hipError_t e, const char* what) {
  if (err) *err = std::string(what) + ": " + hipGetErrorString(e);
  return e == hipErrorOutOfMemory ? LCPC_ERR_NOMEM : LCPC_ERR_HIP;
}
// `c` is an lcpc_ctx* or lcpc_commit_t* (both have .err)
#define HIPCHK(c, call)                                                   \
  do {                                                                    \
    hipError_t e__ = (call);                                              \
    if (e__ != hipSuccess) return lcpc::fail_hip((c) ? &(c)->err : nullptr, e__, #call); \
  } while (0)

// nothing may unwind through the C ABI (include/lcpc_hip.h): every extern "C" body that can allocate runs inside this
#define LCPC_TRY try {
#define LCPC_CATCH(c)                                                     \
  } catch (const std::bad_alloc&) {                                       \
    if (c) (c)->err = "host allocation failed";                          \
    return LCPC_ERR_NOMEM;                                                \
  } catch (const std::exception& ex__) {                                  \
    if (c) (c)->err = ex__.what();                                       \
    return LCPC_ERR_STATE;                                                \
  } catch (...) {                                                         \
    return LCPC_ERR_STATE;                                                \
  }

template <typename T> int dev_alloc(ErrText* err, T** p, size_t bytes) {
  *p = nullptr;
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(p), bytes);
  if (e != hipSuccess) return fail_hip(err, e, "hipMalloc");
  return 0;
}
inline void dev_free(void* p) { if (p) (void)hipFree(p); }
// grow-only device buffer; the requested size is rounded up to 256 bytes so that offsets computed from the capacity
// (collapse partials at the end of scratch) stay 16-byte aligned for the uint4 element accesses
template <typename T> int ensure_dev(ErrText* err, T** p, uint64_t* cap, uint64_t bytes) {
  bytes = (bytes + 255) & ~(uint64_t)255;
  if (bytes > *cap || !*p) {
    dev_free(*p);
    *p = nullptr; *cap = 0;
    int rc = dev_alloc(err, p, (size_t)bytes);
    if (rc) return rc;
    *cap = bytes;
  }
  return 0;
}

inline size_t elem_bytes(const lcpc_ctx* c) { return (size_t)8 * c->L; }
// what the device entry points of the extensions (eval.cpp, fft.cpp, domain.cpp, quot.cpp) ask of their arguments: an element pointer
// aligned for the kernels' widest load, a transform no longer than the field's 2-adicity and the launchers allow
inline bool dev_aligned(const void* p, int L) { return reinterpret_cast<uintptr_t>(p) % (L % 2 ? 8 : 16) == 0; }
inline uint32_t dev_max_log_n(const FieldDesc& f) { return f.S < FFT_MAX_LOG_N ? f.S : FFT_MAX_LOG_N; }
// two ranges of na and nb bytes have a byte in common
inline bool ranges_meet(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}
// n_vecs vectors of 2^log_n elements, in and out, on the device: 1 .. 65535 vectors, aligned, log_n <= dev_max_log_n, fewer than 2^39
// elements (*total), in == out or disjoint
inline bool dev_vectors_ok(const lcpc_ctx* c, const uint64_t* in_dev, const uint64_t* out_dev, uint32_t log_n, uint32_t n_vecs, uint64_t* total) {
  if (!in_dev || !out_dev || n_vecs == 0 || n_vecs > 65535) return false;
  if (!dev_aligned(in_dev, c->L) || !dev_aligned(out_dev, c->L) || log_n > dev_max_log_n(*c->f)) return false;
  *total = (uint64_t)n_vecs << log_n;
  if (*total >= ((uint64_t)1 << 39)) return false;
  return in_dev == out_dev || !ranges_meet(in_dev, *total * elem_bytes(c), out_dev, *total * elem_bytes(c));
}
inline bool is_sha3(const lcpc_ctx* c) { return c->prm.hash == LCPC_HASH_SHA3_256; }
inline bool is_blake2b(const lcpc_ctx* c) { return c->prm.hash == LCPC_HASH_BLAKE2B; }
inline bool is_keccak256(const lcpc_ctx* c) { return c->prm.hash == LCPC_HASH_KECCAK256; }
inline bool is_sha256(const lcpc_ctx* c) { return c->prm.hash == LCPC_HASH_SHA256; }
// BLAKE3 is the only digest whose leaf hash splits into chunks (row batches, row shards); SHA3-256, BLAKE2b, Keccak-256 and SHA-256
// are one serial chain
inline bool is_blake3(const lcpc_ctx* c) { return c->prm.hash == LCPC_HASH_BLAKE3; }
// the serial-chain digest of an encoder that is not BLAKE3's (kernels.h launch_chain_*)
inline ChainHash chain_hash(const lcpc_ctx* c) {
  return is_sha3(c) ? ChainHash::Sha3_256 : is_keccak256(c) ? ChainHash::Keccak256 : is_sha256(c) ? ChainHash::Sha256 : ChainHash::Blake2b;
}
// bytes of one Output<D>: a hashes slot, a root, a path entry (32; BLAKE2b 64)
inline uint32_t digest_len(const lcpc_ctx* c) { return is_blake2b(c) ? 64u : 32u; }
inline uint32_t digest_words(const lcpc_ctx* c) { return digest_len(c) / 4; }
// leaf message = 32 + F * n_rows bytes -> BLAKE3 chunks of 1 KiB
inline uint64_t leaf_chunks(const lcpc_ctx* c, uint64_t n_rows) { return (32 + elem_bytes(c) * n_rows + 1023) / 1024; }

// labels of the transcript (macros.rs:31-34)
extern const uint8_t LBL_DT[7], LBL_PR[7], LBL_PE[7], LBL_CO[7];


// ---- ctx.cpp ----------------------------------------------------------------------------------------
void ctx_ref(lcpc_ctx* c);
void ctx_unref(lcpc_ctx* c);
// encode n_rows rows: src (src_stride elements per row, first n_valid valid, flat elements >= n_src_total zero) -> dst
// (n_cols per row).  err: where HIP error text goes; launches: encode launch counter or null.
struct EncodeJob {
  const uint32_t* src = nullptr;
  uint64_t src_stride = 0, n_valid = 0;
  uint32_t* dst = nullptr;
  uint64_t n_rows = 0;
  uint64_t n_src_total = ~(uint64_t)0;
  uint32_t* copy_dst = nullptr;    // padded LcCommit.coeffs copy written while the source streams through (or null)
  bool canon_out = false;          // dst receives canonical values instead of Montgomery form (commit paths of a comm_canon context)
  bool keep_t = false;             // Brakedown: leave the result position-major in ws->d_t (the commit path); *kept_t reports it
  bool* kept_t = nullptr;
};
int encode_rows_device(const lcpc_ctx* c, EncodeWs* ws, const EncodeJob& j, hipStream_t st, ErrText* err, uint32_t* launches);

int encode_msgs_host(lcpc_ctx* c, const uint64_t* const* msgs, uint64_t n_rows, uint64_t* out);

// The level walk of a Brakedown encode (encode.rs:36-94) over the segments of a codeword: precodes down, the last one into the encode's d_tmp,
// the R-S base case from d_tmp, postcodes up.  mat(m, in_off, out_off, into_tmp) and rs(out_off, n_out) each launch one step
// (ctx.cpp encode_rows_device; batch.cpp over the batch launchers).
template <class Mat, class Rs> int sdig_walk(const lcpc_ctx* c, Mat&& mat, Rs&& rs) {
  const size_t t = c->d_pre.size();
  const DevCsr& pl = c->d_pre[t - 1];
  uint64_t in_start = 0;
  for (size_t i = 0; i + 1 < t; i++) {
    if (int rc = mat(c->d_pre[i], in_start, in_start + c->d_pre[i].n_in, false)) return rc;
    in_start += c->d_pre[i].n_in;
  }
  if (int rc = mat(pl, in_start, 0, true)) return rc;
  const uint64_t in_end = in_start + pl.n_in;
  if (int rc = rs(in_end, c->d_post[t - 1].n_in)) return rc;
  in_start = in_end + pl.n_out;
  uint64_t out_start = in_end + c->d_post[t - 1].n_in;
  for (size_t ii = t; ii-- > 0;) {
    in_start -= c->d_pre[ii].n_out;
    if (int rc = mat(c->d_post[ii], in_start, out_start, false)) return rc;
    out_start += c->d_post[ii].n_out;
  }
  return 0;
}

// ---- commit.cpp -------------------------------------------------------------------------------------
int ensure_scratch(lcpc_commit_t* m, DevScratch* sc, uint64_t bytes);
int ensure_cvs(lcpc_commit_t* m, uint64_t n_chunks);
// The stages of every commit entry point (unsharded: rows [0, n_rows), chunks [0, leaf_chunks(n_rows)); a row shard: its own ranges):
//   begin_commit            st behind the previous fill; every per-commit field reset, the row / chunk range set
//   ensure_commit_buffers   comm_rows: a row-major d_comm even where the commitment would live position-major (from_parts, bincode)
//   encode_coeffs           device source src (n_src elements, the rest of the last row zero) -> comm; coeffs_view / comm_t.
//                           LcCommit.coeffs is the caller's buffer (borrow), the copy the first pass writes, or a copy made first
//   hash_chunks             leaf-message chunks [a, b) of every column -> chaining values out[b - a][n_cols] (one chunk in all: the digests)
//   merkle_top              zero padding leaves + tree above the leaf digests (above level `levels_done`)
//   seal_commit             timings, committed, ev_done; the root -> host when asked for (synchronises st)
int begin_commit(lcpc_commit_t* m, hipStream_t st, uint64_t n_rows_total, uint64_t row_begin, uint64_t row_end, uint64_t chunk_begin,
                 uint64_t chunk_end);
int ensure_commit_buffers(lcpc_commit_t* m, uint64_t n_rows_local, bool own_coeffs, bool comm_rows);
// a member of a batched commit gives up its views of the shared slab (and its share of it): it owns no coeffs / hashes then, and no
// comm or T that was a view (a row-major copy of its own, made by ensure_comm_rows, it keeps)
void leave_slab(lcpc_commit_t* m);
// a row-major d_comm of the member's OWN for the rows it holds (lcpc_get_comm on a position-major commitment); touches nothing else
int ensure_comm_rows(lcpc_commit_t* m);
// hash_columns + merkle_tree of m's commitment matrix, wherever it lives (leaf_args), by the one-shot launchers
int merkleize_device(lcpc_commit_t* m, hipStream_t st);
// lcpc_commit_device behind its argument checks and locks (the caller holds m->fill_mu exclusively and m->mu; the device is current)
int commit_device_locked(lcpc_commit_t* m, const uint64_t* coeffs_dev, uint64_t n_coeffs, hipStream_t st, uint32_t flags, uint8_t* root);
int encode_coeffs(lcpc_commit_t* m, const uint32_t* src, uint64_t n_src, bool borrow, hipStream_t st);
// What a host commit reads: n stored elements (kind < 0: lcpc_commit), or n plain integers of lcpci_kind `kind` that the device widens
// into LcCommit.coeffs behind their upload (lcpci_commit_ints).  One pipeline for both (commit.cpp commit_host_locked)
struct HostSource {
  const void* p = nullptr;
  int kind = -1;
};
// lcpc_commit / lcpci_commit_ints behind their argument checks and locks (as commit_device_locked); complete on return
int commit_host_locked(lcpc_commit_t* m, const HostSource& src, uint64_t n_coeffs, uint8_t* root);
// lcpci_commit_ints_device likewise: widen into LcCommit.coeffs, encode from there
int commit_ints_device_locked(lcpc_commit_t* m, int kind, const void* vals_dev, uint64_t n_coeffs, hipStream_t st, uint8_t* root);
// lcpcf_commit_evals_device / lcpcf_commit_evals (include/lcpc_hip_fft.h) behind their argument checks and locks: the inverse transform
// (form: FFT_IFFT_II or FFT_IFFT_OI) of 2^log_n evaluations lands in LcCommit.coeffs and the pipeline runs from there.  host: `evals` is
// host memory, uploaded into coeffs and transformed in place, and the call is complete on return
// shift (host limbs, checked by the caller) non-null: the values lie on the coset D(shift, 2^log_n) (include/lcpc_hip_domain.h)
int commit_evals_locked(lcpc_commit_t* m, int form, const uint64_t* evals, uint32_t log_n, bool host, hipStream_t st, uint8_t* root,
                        const uint64_t* shift = nullptr);
// K12 / K13 on `st` with the context's twiddle tables (fft.cpp; takes c->mu): in == out in place, otherwise disjoint
int fft_enqueue(lcpc_ctx* c, ErrText* err, int form, const uint32_t* in, uint32_t* out, uint32_t log_n, uint32_t n_vecs, hipStream_t st);
// the four commit-from-evaluations entry points (lcpcf_commit_evals*, lcpcd_commit_coset_evals*) whole, argument checks and locks
// included (fft.cpp).  host: `evals` is host memory and st unused; coset: shift must be a shift (fft_host.h shift_ok), else it is unused
int commit_evals_entry(lcpc_commit_t* m, uint32_t order, bool coset, const uint64_t* shift, const uint64_t* evals, uint32_t log_n, bool host,
                       hipStream_t st, uint8_t* root);
// The context's cached two-level tables, c->mu held (fft.cpp): the table of key (shift, log_n, inverse) among tabs[n_tabs] -- found, or
// built on the host (fft_host.h two_level_table), uploaded and put in place of the entry used longest ago.  shift null: the all-zero key.
// base names what a miss builds from: the base element v and, where it returns true, the factor c of the upper level
using TabBase = bool (*)(const FieldDesc& f, const uint64_t* shift, uint32_t log_n, bool inverse, uint64_t* v, uint64_t* c);
int cached_table(lcpc_ctx* c, ErrText* err, FftTab* tabs, int n_tabs, const uint64_t* shift, uint32_t log_n, bool inverse, TabBase base,
                 const uint32_t** tab);
// the context's twiddle table of (log_n, direction): cached_table on the direction's root
int fft_table(lcpc_ctx* c, ErrText* err, uint32_t log_n, bool inverse, const uint32_t** tab);
// K14 on `st` with the context's twiddle and shift tables (domain.cpp; both take c->mu).  shift: host limbs, nonzero and reduced.
// coset_enqueue: in == out in place, otherwise disjoint.  extend_enqueue: n_vecs coefficient vectors -> their values on D(shift, 2^log_m)
int coset_enqueue(lcpc_ctx* c, ErrText* err, int form, const uint64_t* shift, const uint32_t* in, uint32_t* out, uint32_t log_n,
                  uint32_t n_vecs, hipStream_t st);
int extend_enqueue(lcpc_ctx* c, ErrText* err, const uint64_t* shift, const uint32_t* coeffs, uint64_t n_coeffs, uint32_t log_m, bool natural,
                   uint32_t* out, uint32_t n_vecs, hipStream_t st);
int hash_chunks(lcpc_commit_t* m, uint64_t a, uint64_t b, uint32_t* out, hipStream_t st);
int merkle_top(lcpc_commit_t* m, hipStream_t st, uint32_t levels_done = 0);
int seal_commit(lcpc_commit_t* m, hipStream_t st, uint8_t* root);
int order_after_commit(lcpc_commit_t* m, hipStream_t st);          // st waits for the commit that filled m (event; cheap)
int collapse_run(lcpc_commit_t* m, DevScratch* sc, const uint32_t* d_tensors, uint32_t n_tensors, hipStream_t st, uint32_t* d_polys);
size_t collapse_scratch_bytes(const lcpc_commit_t* m, uint32_t n_tensors);
uint32_t collapse_splits(const lcpc_commit_t* m);                  // row splits of a whole-polynomial collapse (>= 16 rows each)
// the host-entry readers (prove, lcpc_collapse, lcpc_open_columns) run in a working set `ws` of m->sets, taken by take_call_set
// (the caller holds m->fill_mu shared): everything on ws->st, synchronised on that stream or its events
int take_call_set(lcpc_commit_t* m, uint64_t pin_bytes, CallSet** ws);
int collapse_host(lcpc_commit_t* m, CallSet* ws, const uint64_t* tensors, uint32_t n_tensors, uint64_t* polys, uint64_t* polys_canon);
int collapse_host_sliced(lcpc_commit_t* m, CallSet* ws, const uint64_t* tensor, uint64_t* polys, uint64_t* polys_canon, uint64_t* cut_out);
int collapse_wait_slice(lcpc_commit_t* m, CallSet* ws, int s);
int open_columns_host(lcpc_commit_t* m, CallSet* ws, const uint64_t* cols, uint32_t n, uint64_t* col_vals, size_t vals_pitch, uint8_t* paths);
// open_column values / paths into device buffers (either may be null)
int open_columns_device(lcpc_commit_t* m, const uint64_t* d_cols, uint32_t n, uint32_t* d_vals, uint32_t* d_paths, hipStream_t st);

// ---- shard.cpp --------------------------------------------------------------------------------------
void shard_layout_of(const lcpc_ctx* c, uint64_t g, uint64_t n_rows, uint64_t* rb, uint64_t* re, uint64_t* cb, uint64_t* ce, uint64_t* nch);
int shard_nodes(uint64_t c0, uint64_t c1, uint64_t* first, uint32_t* lg);
void shard_chunk_range(uint64_t F, uint64_t n_chunks, uint64_t G, uint64_t g, uint64_t* c0, uint64_t* c1);
void comm_release(lcpc_ctx* c);
// the exchange of a row-sharded prove: every rank contributes `bytes` from send_dev, receives all ranks'
// blocks in rank order in recv_dev
struct ShardXchg {
  uint8_t *send_dev, *recv_dev;
  uint64_t max_bytes;
  lcpc_allgather_fn fn;
  void* user;
  bool stream_ordered = false;     // fn only ENQUEUES the all-gather on the commitment's prove stream (the native RCCL exchange):
                                   // no host synchronisation around it; a caller-supplied fn (torch.distributed, MPI) is host-driven
};
// every device step of a sharded prove runs on the commitment's own stream (prove_stream), ordered behind the commit by an event;
// polys_canon (optional): to_repr of the polynomials, converted on the device; vals_pitch: bytes between the values of
// consecutive opened columns in `vals` (0 = packed)
int prove_stream(lcpc_commit_t* m, hipStream_t* st);
int collapse_sharded(lcpc_commit_t* m, const ShardXchg& x, const uint64_t* tensors_full, uint32_t nt, uint64_t* polys, uint64_t* polys_canon);
int open_sharded(lcpc_commit_t* m, const ShardXchg& x, const uint64_t* cols, uint32_t n, uint64_t* vals, size_t vals_pitch, uint8_t* paths);

// ---- prove.cpp --------------------------------------------------------------------------------------
int prove_impl(lcpc_commit_t* m, const uint64_t* outer, uint64_t n_outer, lcpc_transcript* trw, uint8_t** proof, uint64_t* proof_len,
               uint64_t* cols_opened, const ShardXchg* xchg);
// What the single prove and the batched one (batch.cpp) share.
// bincode 1.3 of WrappedLcEvalProof (lib.rs:550-560): n_cols | p_eval | p_random_vec | columns, every size known up front
struct ProofLayout {
  uint64_t n_cols, np, nr, n_deg, n_open;
  uint32_t path_len;
  size_t pbytes;                   // one polynomial
  size_t dl;                       // each path entry: u64 dl | dl bytes (lib.rs:354-372)
  size_t col_bytes;                // one opened column: u64 nr | values | u64 path_len | entries
  size_t off_eval, off_rand0;      // first element of p_eval / of p_random_vec[0]; p_random_vec[i] at off_rand0 + i * (8 + pbytes)
  size_t head, total;              // the columns start at head; values of column k at head + k * col_bytes + 8
};
ProofLayout proof_layout(const lcpc_ctx* c, uint64_t n_rows);
void proof_write_head(const ProofLayout& pl, uint8_t* out);      // every length prefix in front of the columns
// framing and path of columns [k0, k1); their values are in place already, or (vals non-null, [n_open][nr] elements) copied here
void proof_write_columns(const ProofLayout& pl, uint8_t* out, const uint8_t* paths, const uint64_t* vals, uint64_t k0, uint64_t k1);
// the column challenge (lib.rs:1071-1080)
void draw_columns(Transcript& tr, const lcpc_ctx* c, uint64_t* cols, uint64_t n_open);
double now_ms();
// What the single verify and the batched one (verify_batch.cpp) share.
// A proof's bincode (lib.rs:550-560) read in place: every vector a view into the proof bytes (or into `realigned`, the one copy made of a
// proof handed over at an odd address -- every field of the wire layout sits at a multiple of 8 bytes).
struct ProofView {
  struct Vec { const uint64_t* p = nullptr; uint64_t n = 0; const uint64_t* data() const { return p; } uint64_t size() const { return n; } };   // n: 64-bit words
  struct Path { const uint8_t* p = nullptr; uint64_t n = 0; };   // n entries of (u64 dl, dl bytes): digest k at p + (8 + dl) k + 8
  uint64_t n_cols = 0, n_per_row = 0, n_rows = 0;
  Vec p_eval;
  std::vector<Vec> p_random, cols;
  std::vector<Path> paths;
  std::vector<uint64_t> realigned;
};
// the wire layout, then the checks of lib.rs:845-860 against the encoder and the tensor lengths, in lcpc_verify's order: 0 or the
// LCPC_VERR_* code lcpc_verify returns.  The limbs are not looked at (all_reduced, or the caller's own pass over them).
int parse_proof(const lcpc_ctx* c, const uint8_t* proof, uint64_t proof_len, uint64_t n_outer, uint64_t n_inner, ProofView* out);
// D(in) with the encoder's digest (LCPC_HASH_*): 32 bytes into out, 64 for BLAKE2b
void digest_host(uint32_t hash, const uint8_t* in, size_t len, uint8_t* out);

// ---- verify_batch.cpp: what lcpcv_verify_batch and lcpcp_check_columns (columns.cpp) share --------------------------------------------
// verify_column_path (lib.rs:955-982) on the device for opened columns staged position-major: the leaf digests by the batch forms of the
// column-hash launchers, then the path folds (K8b).  Two calls, because the batched verify knows the drawn column numbers only after
// the transcripts, which run beside the leaf digests.
struct StagedColumns {
  uint32_t* cols;                  // [member][n_open][n_rows] stored (Montgomery) elements, every limb < p; member stride in words
  uint64_t cols_stride_w;          // (whole elements and a multiple of 16 bytes: kernels.h, the batch hash launchers)
  uint32_t* canon;                 // a chained digest over Ft255: room for n_batch * cols_stride_w words, the canonical copy; else unused
  uint32_t* cvs;                   // BLAKE3 leaves of more than one chunk: [member][n_chunks][n_open][8]; else unused
  uint64_t cvs_stride_w;
  uint32_t* digests;               // out: [member][n_open][digest words]
  uint64_t dig_stride_w;
  uint64_t n_open, n_rows;
  uint32_t n_batch;
};
// bytes of the canon and cvs segments a member needs (0: the segment is not used)
uint64_t staged_canon_bytes(const lcpc_ctx* c, uint64_t cols_bytes);
uint64_t staged_cvs_bytes(const lcpc_ctx* c, uint64_t n_open, uint64_t n_rows);
// enqueue on st; *launches (may be null) is advanced by the kernels launched
int enqueue_leaf_digests(lcpc_ctx* c, const StagedColumns& sc, hipStream_t st, uint32_t* launches);
int enqueue_fold_paths(lcpc_ctx* c, const FoldPathsArgs& fa, hipStream_t st, uint32_t* launches);

}  // namespace lcpc
