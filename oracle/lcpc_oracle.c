/*
 * oracle/lcpc_oracle.c -- TEST INFRASTRUCTURE ONLY (checker, never the product).
 *
 * Plain-C CPU restatement of the lcpc-2d commit / prove / verify path of
 * conroi/lcpc (reference mounted at /root/reference; all file:line citations
 * below are into that tree).  It plays two roles:
 *   1. the oracle the HIP path is compared against bit-for-bit (tests/),
 *   2. the "port" CPU baseline timed beside the GPU by bench.py
 *      (OpenMP over rows / 32-column blocks, mirroring the reference's Rayon
 *      split points lcpc-2d/src/lib.rs:648-653, 716-743, 768-783, 1105-1121).
 *
 * PARITY STATUS: **parity unpinned** against a running reference.  The
 * reference is Rust-only, cannot be built in this image (no cargo/rustc, crates
 * un-vendored, no Cargo.lock) and ships no golden vectors (all tests draw from
 * thread_rng()).  Pinned instead, in tests/test_oracle_*.py:
 *   - BLAKE3 / merlin / ChaCha20 against upstream published vectors;
 *   - dims + bincode layout against the reference's 36 published proof sizes
 *     (doc/benchmark-results/ *_pvs.txt);
 *   - every relation the reference's own tests assert (lcpc-2d/src/tests.rs);
 *   - this file against the independent bignum restatement oracle/pyref.py.
 * Third-party conventions restated from their published algorithms are tagged
 * [3P]: ff/ff_derive 0.12 (Montgomery form, to_repr, random), fffft 0.4
 * (root choice, DIF order), rand 0.8 (Uniform), rand_core 0.6 (seed_from_u64),
 * rand_chacha 0.3, merlin 2.0, blake3 1.x, bincode 1.3, sprs 0.10.
 */
#include "lcpc_oracle.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#ifdef _OPENMP
#include <omp.h>
#endif

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint8_t u8;
typedef unsigned __int128 u128;
#define MAXL 4
#define AINL static inline __attribute__((always_inline))

/* ======================================================================
 * Fields: lcpc-test-fields/src/lib.rs:13-59 via #[derive(PrimeField)] [3P]
 * ====================================================================== */
typedef struct {
  int L;
  u64 p[MAXL], r[MAXL], r2[MAXL], rou[MAXL];
  u64 inv;          /* -p^-1 mod 2^64 */
  u64 gen;
  unsigned S, num_bits;
  u64 top_mask;     /* u64::MAX >> REPR_SHAVE_BITS */
} fld_t;

static fld_t FLD[4] = {
  { 1, { 0x46d0760000000001ull }, {0}, {0}, {0}, 0, 10, 0, 0, 0 },
  { 2, { 0x7f2bd90000000001ull, 0x6e754097ba20e0bfull }, {0}, {0}, {0}, 0, 3, 0, 0, 0 },
  { 3, { 0xd246820000000001ull, 0x936888270ceecbcdull, 0x453708aa3fbc8ddaull }, {0}, {0}, {0}, 0, 5, 0, 0, 0 },
  { 4, { 0x02a4f20000000001ull, 0xef73c79086595f30ull, 0xfda9df04b9575969ull, 0x663c799b6e4d2900ull },
    {0}, {0}, {0}, 0, 5, 0, 0, 0 },
};
static int fld_ready = 0;

AINL int ge_p(const u64 *a, const u64 *p, const int L) {
  for (int i = L - 1; i >= 0; i--) {
    if (a[i] > p[i]) return 1;
    if (a[i] < p[i]) return 0;
  }
  return 1;
}
AINL void sub_p(u64 *a, const u64 *p, const int L) {
  u64 br = 0;
  for (int i = 0; i < L; i++) {
    u128 d = (u128)a[i] - p[i] - br;
    a[i] = (u64)d;
    br = (u64)(d >> 64) & 1;
  }
}
/* ff_derive add_assign: plain add (2p < 2^(64L) so no carry-out) then reduce */
AINL void fadd(u64 *o, const u64 *a, const u64 *b, const fld_t *f, const int L) {
  u64 t[MAXL], c = 0;
  for (int i = 0; i < L; i++) {
    u128 s = (u128)a[i] + b[i] + c;
    t[i] = (u64)s;
    c = (u64)(s >> 64);
  }
  if (ge_p(t, f->p, L)) sub_p(t, f->p, L);
  for (int i = 0; i < L; i++) o[i] = t[i];
}
AINL void fsub(u64 *o, const u64 *a, const u64 *b, const fld_t *f, const int L) {
  u64 t[MAXL], br = 0;
  for (int i = 0; i < L; i++) {
    u128 d = (u128)a[i] - b[i] - br;
    t[i] = (u64)d;
    br = (u64)(d >> 64) & 1;
  }
  if (br) {
    u64 c = 0;
    for (int i = 0; i < L; i++) {
      u128 s = (u128)t[i] + f->p[i] + c;
      t[i] = (u64)s;
      c = (u64)(s >> 64);
    }
  }
  for (int i = 0; i < L; i++) o[i] = t[i];
}
/* Montgomery product a*b*R^-1 mod p, fully reduced (ff_derive mul_assign + mont_reduce [3P]) */
AINL void fmul(u64 *o, const u64 *a, const u64 *b, const fld_t *f, const int L) {
  u64 t[MAXL + 2];
  for (int i = 0; i < L + 2; i++) t[i] = 0;
  for (int i = 0; i < L; i++) {
    u64 c = 0;
    for (int j = 0; j < L; j++) {
      u128 s = (u128)a[i] * b[j] + t[j] + c;
      t[j] = (u64)s;
      c = (u64)(s >> 64);
    }
    u128 s = (u128)t[L] + c;
    t[L] = (u64)s;
    t[L + 1] = (u64)(s >> 64);
    u64 m = t[0] * f->inv;
    s = (u128)m * f->p[0] + t[0];
    c = (u64)(s >> 64);
    for (int j = 1; j < L; j++) {
      s = (u128)m * f->p[j] + t[j] + c;
      t[j - 1] = (u64)s;
      c = (u64)(s >> 64);
    }
    s = (u128)t[L] + c;
    t[L - 1] = (u64)s;
    t[L] = t[L + 1] + (u64)(s >> 64);
  }
  if (t[L] || ge_p(t, f->p, L)) sub_p(t, f->p, L);
  for (int i = 0; i < L; i++) o[i] = t[i];
}
AINL void fcopy(u64 *o, const u64 *a, const int L) { for (int i = 0; i < L; i++) o[i] = a[i]; }
AINL int fis_zero(const u64 *a, const int L) { u64 x = 0; for (int i = 0; i < L; i++) x |= a[i]; return x == 0; }
AINL int feq(const u64 *a, const u64 *b, const int L) { u64 x = 0; for (int i = 0; i < L; i++) x |= a[i] ^ b[i]; return x == 0; }
/* to_repr: Montgomery -> canonical (multiply by 1), little-endian limbs (= LE bytes on this host) */
AINL void fcanon(u64 *o, const u64 *a, const fld_t *f, const int L) {
  u64 one[MAXL] = { 1, 0, 0, 0 };
  fmul(o, a, one, f, L);
}

static void fld_init(void) {
  if (fld_ready) return;
  for (int k = 0; k < 4; k++) {
    fld_t *f = &FLD[k];
    const int L = f->L;
    /* inv = -p^-1 mod 2^64 (Newton) */
    u64 x = 1;
    for (int i = 0; i < 6; i++) x *= 2 - f->p[0] * x;
    f->inv = (u64)0 - x;
    /* R, R^2 by repeated doubling mod p */
    u64 t[MAXL] = { 1, 0, 0, 0 };
    for (int rep = 0; rep < 2; rep++) {
      for (int i = 0; i < 64 * L; i++) fadd(t, t, t, f, L);
      fcopy(rep == 0 ? f->r : f->r2, t, L);
    }
    /* bit length, two-adicity */
    int top = L - 1;
    unsigned nb = 64 * top;
    for (u64 v = f->p[top]; v; v >>= 1) nb++;
    f->num_bits = nb;
    f->top_mask = (~(u64)0) >> (64 * L - nb);
    u64 e[MAXL];
    fcopy(e, f->p, L);
    e[0] -= 1;
    unsigned S = 0;
    while ((e[0] & 1) == 0) {
      for (int i = 0; i < L; i++) e[i] = (e[i] >> 1) | (i + 1 < L ? e[i + 1] << 63 : 0);
      S++;
    }
    f->S = S;
    /* root_of_unity = gen^((p-1)/2^S), in Montgomery form */
    u64 g[MAXL] = { f->gen, 0, 0, 0 }, acc[MAXL];
    fmul(g, g, f->r2, f, L);
    fcopy(acc, f->r, L);
    for (int bit = 64 * L - 1; bit >= 0; bit--) {
      fmul(acc, acc, acc, f, L);
      if ((e[bit / 64] >> (bit % 64)) & 1) fmul(acc, acc, g, f, L);
    }
    fcopy(f->rou, acc, L);
  }
  fld_ready = 1;
}
static const fld_t *getf(int fid) {
  if (fid < 0 || fid > 3) return NULL;
  fld_init();
  return &FLD[fid];
}

int lo_field_limbs(int fid) { const fld_t *f = getf(fid); return f ? f->L : LO_ERR_ARG; }
int lo_field_info(int fid, u64 *modulus, u64 *r, u64 *r2, u64 *inv, u64 *rou, u32 *S, u32 *nb) {
  const fld_t *f = getf(fid);
  if (!f) return LO_ERR_ARG;
  if (modulus) fcopy(modulus, f->p, f->L);
  if (r) fcopy(r, f->r, f->L);
  if (r2) fcopy(r2, f->r2, f->L);
  if (inv) *inv = f->inv;
  if (rou) fcopy(rou, f->rou, f->L);
  if (S) *S = f->S;
  if (nb) *nb = f->num_bits;
  return 0;
}
#define DISPATCH_L(f, ...) switch ((f)->L) { case 1: { enum { L = 1 }; __VA_ARGS__; } break; \
  case 2: { enum { L = 2 }; __VA_ARGS__; } break; case 3: { enum { L = 3 }; __VA_ARGS__; } break; \
  default: { enum { L = 4 }; __VA_ARGS__; } break; }

void lo_f_mul(int fid, const u64 *a, const u64 *b, u64 *o, size_t n) {
  const fld_t *f = getf(fid);
  DISPATCH_L(f, for (size_t i = 0; i < n; i++) fmul(o + i * L, a + i * L, b + i * L, f, L));
}
void lo_f_add(int fid, const u64 *a, const u64 *b, u64 *o, size_t n) {
  const fld_t *f = getf(fid);
  DISPATCH_L(f, for (size_t i = 0; i < n; i++) fadd(o + i * L, a + i * L, b + i * L, f, L));
}
void lo_f_sub(int fid, const u64 *a, const u64 *b, u64 *o, size_t n) {
  const fld_t *f = getf(fid);
  DISPATCH_L(f, for (size_t i = 0; i < n; i++) fsub(o + i * L, a + i * L, b + i * L, f, L));
}
void lo_f_to_repr(int fid, const u64 *a, u8 *out, size_t n) {
  const fld_t *f = getf(fid);
  DISPATCH_L(f, for (size_t i = 0; i < n; i++) { u64 t[MAXL]; fcanon(t, a + i * L, f, L); memcpy(out + 8 * L * i, t, 8 * L); });
}
void lo_f_from_canon(int fid, const u64 *c, u64 *o, size_t n) {
  const fld_t *f = getf(fid);
  DISPATCH_L(f, for (size_t i = 0; i < n; i++) fmul(o + i * L, c + i * L, f->r2, f, L));
}
void lo_f_from_u64(int fid, const u64 *v, u64 *o, size_t n) {
  const fld_t *f = getf(fid);
  DISPATCH_L(f, for (size_t i = 0; i < n; i++) { u64 t[MAXL] = { v[i], 0, 0, 0 }; if (L == 1 && t[0] >= f->p[0]) t[0] %= f->p[0]; fmul(o + i * L, t, f->r2, f, L); });
}

/* ======================================================================
 * NTT: lcpc-ligero-pc/src/lib.rs:162-164 -> fffft::FieldFFT::fft_io_pc [3P]
 * ====================================================================== */
int lo_roots_table(int fid, unsigned log_n, u64 *out) {
  const fld_t *f = getf(fid);
  if (!f || log_n > f->S) return LO_ERR_ARG;
  const int L = f->L;
  /* w = ROOT_OF_UNITY^(2^(S-log_n)); roots[i] = w^i, i < n/2 (fffft precomp_fft [3P]) */
  u64 w[MAXL];
  fcopy(w, f->rou, L);
  for (unsigned i = 0; i < f->S - log_n; i++) fmul(w, w, w, f, L);
  size_t half = log_n == 0 ? 1 : ((size_t)1 << log_n) / 2;
  fcopy(out, f->r, L);
  for (size_t i = 1; i < half; i++) fmul(out + i * L, out + (i - 1) * L, w, f, L);
  return 0;
}
AINL void fft_io_L(u64 *x, size_t n, const u64 *roots, const fld_t *f, const int L) {
  /* radix-2 DIF, natural in, bit-reversed out, no final permutation (fffft io_help [3P]) */
  for (size_t gap = n / 2; gap > 0; gap /= 2) {
    size_t nchunks = n / (2 * gap);
    for (size_t c = 0; c < nchunks; c++) {
      u64 *lo = x + 2 * c * gap * L, *hi = lo + gap * L;
      for (size_t idx = 0; idx < gap; idx++) {
        u64 neg[MAXL];
        fsub(neg, lo + idx * L, hi + idx * L, f, L);
        fadd(lo + idx * L, lo + idx * L, hi + idx * L, f, L);
        fmul(hi + idx * L, neg, roots + nchunks * idx * L, f, L);
      }
    }
  }
}
static void fft_io_pc(const fld_t *f, u64 *x, size_t n, const u64 *roots) {
  DISPATCH_L(f, fft_io_L(x, n, roots, f, L));
}
int lo_fft_io(int fid, u64 *x, unsigned log_n) {
  const fld_t *f = getf(fid);
  if (!f || log_n > f->S) return LO_ERR_ARG;
  size_t n = (size_t)1 << log_n;
  u64 *roots = malloc((n / 2 + 1) * f->L * 8);
  lo_roots_table(fid, log_n, roots);
  fft_io_pc(f, x, n, roots);
  free(roots);
  return 0;
}
/* a / 2 mod p of a fully reduced a (either form: halving is linear) */
AINL void fhalf(u64 *a, const fld_t *f, const int L) {
  u64 c = 0;
  if (a[0] & 1) {
    for (int i = 0; i < L; i++) {
      u128 s = (u128)a[i] + f->p[i] + c;
      a[i] = (u64)s;
      c = (u64)(s >> 64);
    }
  }
  for (int i = 0; i < L; i++) a[i] = (a[i] >> 1) | (i + 1 < L ? a[i + 1] << 63 : c << 63);
}
static void fpow_u64(u64 *o, const u64 *b, u64 e, const fld_t *f, const int L) {
  u64 acc[MAXL], sq[MAXL];
  fcopy(acc, f->r, L);
  fcopy(sq, b, L);
  for (; e; e >>= 1) {
    if (e & 1) fmul(acc, acc, sq, f, L);
    fmul(sq, sq, sq, f, L);
  }
  fcopy(o, acc, L);
}
AINL void dif_stage_L(u64 *x, u64 len, u64 gap, const u64 *b, int inverse, int nthreads, const fld_t *f, const int L) {
  u64 *tw = malloc(gap * L * 8);
  const u64 CH = 1024;
#pragma omp parallel for schedule(static) num_threads(nthreads)
  for (u64 c = 0; c < (gap + CH - 1) / CH; c++) {
    const u64 i0 = c * CH, i1 = i0 + CH < gap ? i0 + CH : gap;
    fpow_u64(tw + i0 * L, b, i0, f, L);
    for (u64 i = i0 + 1; i < i1; i++) fmul(tw + i * L, tw + (i - 1) * L, b, f, L);
  }
#pragma omp parallel for schedule(static) num_threads(nthreads)
  for (u64 j = 0; j < len / 2; j++) {
    const u64 i = j % gap;
    u64 *lo = x + ((j / gap) * 2 * gap + i) * L, *hi = lo + gap * L;
    u64 t[MAXL];
    if (inverse) {
      fmul(t, hi, tw + i * L, f, L);
      fsub(hi, lo, t, f, L);
      fadd(lo, lo, t, f, L);
      fhalf(lo, f, L);
      fhalf(hi, f, L);
    } else {
      fsub(t, lo, hi, f, L);
      fadd(lo, lo, hi, f, L);
      fmul(hi, t, tw + i * L, f, L);
    }
  }
  free(tw);
}
/* stage k of fft_io_L for a length-2^log_n transform (gap = 2^log_n >> (k + 1), lo' = lo + hi, hi' = (lo - hi) w^(2^k idx)), or
 * its inverse, in place over len elements: consecutive blocks of 2 gap (a whole row, a prefix of one made of whole blocks, or
 * many rows back to back).  Test infrastructure: the stage-input builder of tests/common.py. */
int lo_dif_stage(int fid, u64 *x, u64 len, unsigned log_n, unsigned k, int inverse, int nthreads) {
  const fld_t *f = getf(fid);
  if (!f || log_n > f->S || k >= log_n) return LO_ERR_ARG;
  const u64 gap = ((u64)1 << log_n) >> (k + 1);
  if (len % (2 * gap)) return LO_ERR_ARG;
  const int L = f->L;
  u64 b[MAXL];                                   /* w^(2^k), of order 2 gap; its inverse is its (2 gap - 1)-th power */
  fcopy(b, f->rou, L);
  for (unsigned i = 0; i < f->S - log_n + k; i++) fmul(b, b, b, f, L);
  if (inverse) fpow_u64(b, b, 2 * gap - 1, f, L);
  DISPATCH_L(f, dif_stage_L(x, len, gap, b, inverse, nthreads > 0 ? nthreads : 1, f, L));
  return 0;
}

/* ======================================================================
 * BLAKE3 (plain hash mode) [3P] -- the D: Digest of every reference test
 * (lcpc-ligero-pc/src/tests.rs:12); streaming update()/finalize()
 * ====================================================================== */
static const u32 B3_IV[8] = { 0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19 };
static const u8 B3_PERM[16] = { 2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8 };
enum { B3_CHUNK_START = 1, B3_CHUNK_END = 2, B3_PARENT = 4, B3_ROOT = 8 };
AINL u32 rotr32(u32 x, int n) { return (x >> n) | (x << (32 - n)); }
#define B3G(a, b, c, d, mx, my) \
  s[a] = s[a] + s[b] + (mx); s[d] = rotr32(s[d] ^ s[a], 16); s[c] = s[c] + s[d]; s[b] = rotr32(s[b] ^ s[c], 12); \
  s[a] = s[a] + s[b] + (my); s[d] = rotr32(s[d] ^ s[a], 8);  s[c] = s[c] + s[d]; s[b] = rotr32(s[b] ^ s[c], 7);
static void b3_compress(u32 cv[8], const u32 block[16], u64 counter, u32 blen, u32 flags) {
  u32 s[16], m[16], t[16];
  for (int i = 0; i < 8; i++) s[i] = cv[i];
  for (int i = 0; i < 4; i++) s[8 + i] = B3_IV[i];
  s[12] = (u32)counter; s[13] = (u32)(counter >> 32); s[14] = blen; s[15] = flags;
  for (int i = 0; i < 16; i++) m[i] = block[i];
  for (int r = 0; r < 7; r++) {
    B3G(0, 4, 8, 12, m[0], m[1]) B3G(1, 5, 9, 13, m[2], m[3]) B3G(2, 6, 10, 14, m[4], m[5]) B3G(3, 7, 11, 15, m[6], m[7])
    B3G(0, 5, 10, 15, m[8], m[9]) B3G(1, 6, 11, 12, m[10], m[11]) B3G(2, 7, 8, 13, m[12], m[13]) B3G(3, 4, 9, 14, m[14], m[15])
    for (int i = 0; i < 16; i++) t[i] = m[B3_PERM[i]];
    for (int i = 0; i < 16; i++) m[i] = t[i];
  }
  for (int i = 0; i < 8; i++) cv[i] = s[i] ^ s[i + 8];
}
typedef struct {
  u32 cv[8];           /* current chunk chaining value */
  u8 buf[64];
  u32 buf_len, blocks_done;
  u64 chunk_counter;
  u32 stack[54][8];
  int stack_len;
} b3_t;
static void b3_init(b3_t *h) {
  memcpy(h->cv, B3_IV, 32);
  h->buf_len = 0; h->blocks_done = 0; h->chunk_counter = 0; h->stack_len = 0;
}
static void b3_push_cv(b3_t *h, u32 cv[8], u64 total_chunks) {
  while ((total_chunks & 1) == 0) {
    u32 blk[16];
    memcpy(blk, h->stack[--h->stack_len], 32);
    memcpy(blk + 8, cv, 32);
    memcpy(cv, B3_IV, 32);
    b3_compress(cv, blk, 0, 64, B3_PARENT);
    total_chunks >>= 1;
  }
  memcpy(h->stack[h->stack_len++], cv, 32);
}
static void b3_update(b3_t *h, const u8 *in, size_t len) {
  while (len > 0) {
    if (h->buf_len == 64) {
      /* buffer full and more input follows => this is not the last block of the message */
      u32 blk[16];
      memcpy(blk, h->buf, 64);
      u32 flags = h->blocks_done == 0 ? B3_CHUNK_START : 0;
      if (h->blocks_done == 15) {
        flags |= B3_CHUNK_END;
        b3_compress(h->cv, blk, h->chunk_counter, 64, flags);
        u32 cv[8];
        memcpy(cv, h->cv, 32);
        h->chunk_counter++;
        b3_push_cv(h, cv, h->chunk_counter);
        memcpy(h->cv, B3_IV, 32);
        h->blocks_done = 0;
      } else {
        b3_compress(h->cv, blk, h->chunk_counter, 64, flags);
        h->blocks_done++;
      }
      h->buf_len = 0;
    }
    size_t take = 64 - h->buf_len;
    if (take > len) take = len;
    memcpy(h->buf + h->buf_len, in, take);
    h->buf_len += take; in += take; len -= take;
  }
}
static void b3_final(const b3_t *h, u8 out[32]) {
  u32 blk[16] = { 0 }, cv[8];
  memcpy(blk, h->buf, h->buf_len);
  memcpy(cv, h->cv, 32);
  u32 flags = (h->blocks_done == 0 ? B3_CHUNK_START : 0) | B3_CHUNK_END;
  if (h->stack_len == 0) {
    b3_compress(cv, blk, h->chunk_counter, h->buf_len, flags | B3_ROOT);
  } else {
    b3_compress(cv, blk, h->chunk_counter, h->buf_len, flags);
    for (int i = h->stack_len - 1; i >= 0; i--) {
      u32 pb[16];
      memcpy(pb, h->stack[i], 32);
      memcpy(pb + 8, cv, 32);
      memcpy(cv, B3_IV, 32);
      b3_compress(cv, pb, 0, 64, B3_PARENT | (i == 0 ? B3_ROOT : 0));
    }
  }
  memcpy(out, cv, 32);
}
void lo_blake3(const u8 *in, size_t len, u8 out[32]) {
  b3_t h;
  b3_init(&h);
  b3_update(&h, in, len);
  b3_final(&h, out);
}

/* ======================================================================
 * Keccak-f[1600] / STROBE-128 / merlin::Transcript 2.0 [3P]
 * (call sites lcpc-2d/src/lib.rs:47-49, 871, 904, 1027, 1074)
 * ====================================================================== */
AINL u64 rol64(u64 x, int n) { return n ? (x << n) | (x >> (64 - n)) : x; }
void lo_keccak_f1600(u8 state[200]) {
  static const u64 RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull,
    0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull,
    0x0000000080008009ull, 0x000000008000000Aull, 0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull,
    0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
    0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull };
  static const int ROT[25] = { 0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14 };
  u64 a[25], b[25], c[5], d[5];
  memcpy(a, state, 200);
  for (int r = 0; r < 24; r++) {
    for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
    for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ rol64(c[(x + 1) % 5], 1);
    for (int i = 0; i < 25; i++) a[i] ^= d[i % 5];
    for (int x = 0; x < 5; x++)
      for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = rol64(a[x + 5 * y], ROT[x + 5 * y]);
    for (int y = 0; y < 5; y++)
      for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
    a[0] ^= RC[r];
  }
  memcpy(state, a, 200);
}
#define STROBE_R 166
enum { SF_I = 1, SF_A = 2, SF_C = 4, SF_T = 8, SF_M = 16, SF_K = 32 };
struct lo_transcript { u8 st[200]; u8 pos, pos_begin, cur_flags; };
static void strobe_run_f(lo_transcript *s) {
  s->st[s->pos] ^= s->pos_begin;
  s->st[s->pos + 1] ^= 0x04;
  s->st[STROBE_R + 1] ^= 0x80;
  lo_keccak_f1600(s->st);
  s->pos = 0; s->pos_begin = 0;
}
static void strobe_absorb(lo_transcript *s, const u8 *d, size_t n) {
  for (size_t i = 0; i < n; i++) {
    s->st[s->pos++] ^= d[i];
    if (s->pos == STROBE_R) strobe_run_f(s);
  }
}
static void strobe_squeeze(lo_transcript *s, u8 *d, size_t n) {
  for (size_t i = 0; i < n; i++) {
    d[i] = s->st[s->pos];
    s->st[s->pos++] = 0;
    if (s->pos == STROBE_R) strobe_run_f(s);
  }
}
static void strobe_begin_op(lo_transcript *s, u8 flags, int more) {
  if (more) return;
  u8 hdr[2] = { s->pos_begin, flags };
  s->pos_begin = s->pos + 1;
  s->cur_flags = flags;
  strobe_absorb(s, hdr, 2);
  if ((flags & (SF_C | SF_K)) && s->pos != 0) strobe_run_f(s);
}
static void strobe_meta_ad(lo_transcript *s, const u8 *d, size_t n, int more) { strobe_begin_op(s, SF_M | SF_A, more); strobe_absorb(s, d, n); }
static void strobe_ad(lo_transcript *s, const u8 *d, size_t n, int more) { strobe_begin_op(s, SF_A, more); strobe_absorb(s, d, n); }
static void strobe_prf(lo_transcript *s, u8 *d, size_t n, int more) { strobe_begin_op(s, SF_I | SF_A | SF_C, more); strobe_squeeze(s, d, n); }
void lo_tr_append_message(lo_transcript *t, const u8 *label, size_t llen, const u8 *msg, size_t mlen) {
  u32 l32 = (u32)mlen;
  u8 le[4] = { (u8)l32, (u8)(l32 >> 8), (u8)(l32 >> 16), (u8)(l32 >> 24) };
  strobe_meta_ad(t, label, llen, 0);
  strobe_meta_ad(t, le, 4, 1);
  strobe_ad(t, msg, mlen, 0);
}
void lo_tr_challenge_bytes(lo_transcript *t, const u8 *label, size_t llen, u8 *out, size_t n) {
  u32 l32 = (u32)n;
  u8 le[4] = { (u8)l32, (u8)(l32 >> 8), (u8)(l32 >> 16), (u8)(l32 >> 24) };
  strobe_meta_ad(t, label, llen, 0);
  strobe_meta_ad(t, le, 4, 1);
  strobe_prf(t, out, n, 0);
}
lo_transcript *lo_tr_new(const u8 *label, size_t len) {
  lo_transcript *t = calloc(1, sizeof *t);
  static const u8 hdr[6] = { 1, STROBE_R + 2, 1, 0, 1, 96 };
  memcpy(t->st, hdr, 6);
  memcpy(t->st + 6, "STROBEv1.0.2", 12);
  lo_keccak_f1600(t->st);
  strobe_meta_ad(t, (const u8 *)"Merlin v1.0", 11, 0);
  lo_tr_append_message(t, (const u8 *)"dom-sep", 7, label, len);
  return t;
}
lo_transcript *lo_tr_clone(const lo_transcript *t) { lo_transcript *c = malloc(sizeof *c); *c = *t; return c; }
void lo_tr_free(lo_transcript *t) { free(t); }

/* ======================================================================
 * ChaCha20Rng (rand_chacha 0.3), seed_from_u64 (rand_core 0.6),
 * Uniform<usize> (rand 0.8), Field::random (ff_derive) -- all [3P]
 * ====================================================================== */
struct lo_rng { u32 key[8]; u64 counter, stream; u32 buf[64]; int idx; };
#define QR(a, b, c, d) x[a] += x[b]; x[d] = rotr32(x[d] ^ x[a], 16); x[c] += x[d]; x[b] = rotr32(x[b] ^ x[c], 20); \
  x[a] += x[b]; x[d] = rotr32(x[d] ^ x[a], 24); x[c] += x[d]; x[b] = rotr32(x[b] ^ x[c], 25);
static void chacha_block(const lo_rng *g, u64 counter, u32 out[16]) {
  u32 st[16] = { 0x61707865, 0x3320646E, 0x79622D32, 0x6B206574 }, x[16];
  for (int i = 0; i < 8; i++) st[4 + i] = g->key[i];
  st[12] = (u32)counter; st[13] = (u32)(counter >> 32); st[14] = (u32)g->stream; st[15] = (u32)(g->stream >> 32);
  memcpy(x, st, 64);
  for (int r = 0; r < 10; r++) {
    QR(0, 4, 8, 12) QR(1, 5, 9, 13) QR(2, 6, 10, 14) QR(3, 7, 11, 15)
    QR(0, 5, 10, 15) QR(1, 6, 11, 12) QR(2, 7, 8, 13) QR(3, 4, 9, 14)
  }
  for (int i = 0; i < 16; i++) out[i] = x[i] + st[i];
}
static void rng_refill(lo_rng *g) {
  for (int b = 0; b < 4; b++) chacha_block(g, g->counter++, g->buf + 16 * b);
  g->idx = 0;
}
lo_rng *lo_rng_from_seed(const u8 seed[32]) {
  lo_rng *g = calloc(1, sizeof *g);
  memcpy(g->key, seed, 32);
  g->idx = 64;
  return g;
}
lo_rng *lo_rng_seed_from_u64(u64 state) {
  u8 seed[32];
  for (int i = 0; i < 8; i++) {
    state = state * 6364136223846793005ull + 11634580027462260723ull;
    u32 xs = (u32)(((state >> 18) ^ state) >> 27);
    u32 rot = (u32)(state >> 59);
    u32 x = rot ? rotr32(xs, rot) : xs;
    memcpy(seed + 4 * i, &x, 4);
  }
  return lo_rng_from_seed(seed);
}
void lo_rng_set_stream(lo_rng *g, u64 s) { g->stream = s; }
u32 lo_rng_next_u32(lo_rng *g) {
  if (g->idx >= 64) rng_refill(g);
  return g->buf[g->idx++];
}
u64 lo_rng_next_u64(lo_rng *g) {
  /* rand_core BlockRng::next_u64 */
  u64 lo, hi;
  if (g->idx < 63) { lo = g->buf[g->idx]; hi = g->buf[g->idx + 1]; g->idx += 2; }
  else if (g->idx >= 64) { rng_refill(g); lo = g->buf[0]; hi = g->buf[1]; g->idx = 2; }
  else { lo = g->buf[63]; rng_refill(g); hi = g->buf[0]; g->idx = 1; }
  return lo | (hi << 32);
}
u64 lo_rng_uniform(lo_rng *g, u64 range) {
  u64 ints_to_reject = (UINT64_MAX - range + 1) % range;
  u64 zone = UINT64_MAX - ints_to_reject;
  for (;;) {
    u64 v = lo_rng_next_u64(g);
    u128 m = (u128)v * range;
    if ((u64)m <= zone) return (u64)(m >> 64);
  }
}
static void rng_field_random1(lo_rng *g, const fld_t *f, u64 *out) {
  for (;;) {
    for (int i = 0; i < f->L; i++) out[i] = lo_rng_next_u64(g);
    out[f->L - 1] &= f->top_mask;
    if (!ge_p(out, f->p, f->L)) return;     /* accepted limbs ARE the Montgomery repr */
  }
}
void lo_rng_field_random(lo_rng *g, int fid, u64 *out, size_t n) {
  const fld_t *f = getf(fid);
  for (size_t i = 0; i < n; i++) rng_field_random1(g, f, out + i * f->L);
}
void lo_rng_free(lo_rng *g) { free(g); }

/* ======================================================================
 * Encodings
 * ====================================================================== */
static u64 log2c(u64 v) { /* lcpc-2d/src/lib.rs:827-829 */ u64 l = 0; while (((u64)1 << l) < v) l++; return l; }
static u64 np2(u64 v) { return (u64)1 << log2c(v); }
static u64 n_degree_tests(u64 lambda, u64 len, u64 flog2) { /* lib.rs:613-616 */
  u64 den = flog2 - log2c(len);
  return (lambda + den - 1) / den;
}

typedef struct { u64 rows, cols, nnz; u64 *colptr, *rowidx, *vals; } csc_t;
struct lo_enc {
  int kind, fid;
  const fld_t *f;
  u64 n_per_row, n_cols;
  unsigned rho_num, rho_den;     /* ligero */
  u64 *roots;
  int code, n_levels;            /* sdig */
  u64 seed;
  csc_t *pre, *post;
};

/* ---- Ligero: lcpc-ligero-pc/src/lib.rs:45-148 ---- */
static u64 ligero_n_col_opens(unsigned rn, unsigned rd) { /* lib.rs:61-64 */
  double rho = (double)rn / (double)rd;
  double den = log2((1.0 + rho) / 2.0);
  return (u64)ceil(-128.0 / den);
}
int lo_ligero_get_dims(int fid, u64 len, unsigned rn, unsigned rd, u64 *nr, u64 *np, u64 *nc) { /* lib.rs:70-112 */
  const fld_t *f = getf(fid);
  if (!f || rn >= rd || len == 0) return LO_ERR_ARG;
  double rho = (double)rn / (double)rd;
  u64 flog2 = f->num_bits - 1;
  u64 n_col_opens = ligero_n_col_opens(rn, rd);
  double lncf = (double)(n_col_opens * len);
  double ndt = (double)n_degree_tests(128, (u64)ceil(sqrt(lncf) / rho), flog2);
  u64 nc1 = np2((u64)ceil(sqrt(lncf / ndt) / rho));
  if (nc1 > ((u64)1 << f->S)) return LO_ERR_TOO_BIG;
  u64 np1 = nc1 * rn / rd, nr1 = (len + np1 - 1) / np1, nd1 = n_degree_tests(128, nc1, flog2);
  u64 nc2 = nc1 / 2, np2_ = np1 / 2, nr2 = (len + np2_ - 1) / np2_, nd2 = n_degree_tests(128, nc2, flog2);
  u64 sz1 = n_col_opens * nr1 + (1 + nd1) * np1, sz2 = n_col_opens * nr2 + (1 + nd2) * np2_;
  if (sz1 < sz2) { *nr = nr1; *np = np1; *nc = nc1; } else { *nr = nr2; *np = np2_; *nc = nc2; }
  return 0;
}
lo_enc *lo_ligero_new_from_dims(int fid, u64 n_per_row, u64 n_cols, unsigned rn, unsigned rd) { /* lib.rs:138-148 */
  const fld_t *f = getf(fid);
  if (!f || !(n_per_row < n_cols) || (n_cols & (n_cols - 1)) || log2c(n_cols) > f->S) return NULL;
  lo_enc *e = calloc(1, sizeof *e);
  e->kind = LO_ENC_LIGERO; e->fid = fid; e->f = f; e->n_per_row = n_per_row; e->n_cols = n_cols;
  e->rho_num = rn; e->rho_den = rd;
  e->roots = malloc((n_cols / 2 + 1) * f->L * 8);
  lo_roots_table(fid, (unsigned)log2c(n_cols), e->roots);
  return e;
}
lo_enc *lo_ligero_new(int fid, u64 len, unsigned rn, unsigned rd) { /* lib.rs:121-124 */
  u64 nr, np, nc;
  if (lo_ligero_get_dims(fid, len, rn, rd, &nr, &np, &nc)) return NULL;
  return lo_ligero_new_from_dims(fid, np, nc, rn, rd);
}

/* ---- Brakedown / SDIG: codespec.rs, matgen.rs, encode.rs, lib.rs ---- */
typedef struct { u64 an, ad, bn, bd, rn, rd, baselen; double alpha, beta, r, dist, mu, nu, cn1, cn2, dn1, dn2; } sdig_spec;
static double ent(double z) { return -z * log2(z) - (1.0 - z) * log2(1.0 - z); } /* codespec.rs:17-21 */
static int sdig_spec_get(int code, sdig_spec *s) { /* codespec.rs:24-129, 169-232 */
  static const u64 T[6][7] = { { 239, 2000, 71, 2500, 71, 50, 20 }, { 69, 500, 111, 2500, 147, 100, 20 },
    { 89, 500, 61, 1000, 1521, 1000, 20 }, { 1, 5, 41, 500, 41, 25, 20 }, { 211, 1000, 97, 1000, 202, 125, 20 },
    { 119, 500, 241, 2000, 43, 25, 20 } };
  if (code < 1 || code > 6) return -1;
  const u64 *t = T[code - 1];
  s->an = t[0]; s->ad = t[1]; s->bn = t[2]; s->bd = t[3]; s->rn = t[4]; s->rd = t[5]; s->baselen = t[6];
  s->alpha = (double)s->an / (double)s->ad; s->beta = (double)s->bn / (double)s->bd; s->r = (double)s->rn / (double)s->rd;
  s->dist = (double)(s->bn * s->rd) / (double)(s->bd * s->rn);
  s->mu = s->r - 1.0 - s->r * s->alpha;
  s->nu = s->beta + s->alpha * s->beta + 0.03;
  s->cn1 = ent(s->beta) + s->alpha * ent(1.28 * s->beta / s->alpha);
  s->cn2 = s->beta * log2(s->alpha / (1.28 * s->beta));
  s->dn1 = s->r * s->alpha * ent(s->beta / s->r) + s->mu * ent(s->nu / s->mu);
  s->dn2 = s->alpha * s->beta * log2(s->mu / s->nu);
  return 0;
}
static u64 cmd(u64 n, u64 num, u64 den) { return (n * num + den - 1) / den; } /* matgen.rs:23-25 */
static u64 umin(u64 a, u64 b) { return a < b ? a : b; }
static u64 umax(u64 a, u64 b) { return a > b ? a : b; }
#define MAXLEV 64
/* matgen.rs:56-111; returns number of levels */
static int sdig_get_dims(const sdig_spec *s, u64 n, double log2p, u64 pre[][3], u64 post[][3]) {
  if (n <= s->baselen) return -1;
  u64 tmp[MAXLEV + 1];
  int cnt = 0;
  for (u64 ni = n; ni > s->baselen; ni = cmd(ni, s->an, s->ad)) tmp[cnt++] = ni;
  tmp[cnt] = cmd(tmp[cnt - 1], s->an, s->ad);
  for (int i = 0; i < cnt; i++) {
    u64 ni = tmp[i], mi = tmp[i + 1];
    u64 cn = umin(umax(cmd(ni, 32 * s->bn, 25 * s->bd), 4 + cmd(ni, s->bn, s->bd)),
                  (u64)ceil((110.0 / (double)ni + s->cn1) / s->cn2));
    cn = umin(cn, mi);
    pre[i][0] = ni; pre[i][1] = mi; pre[i][2] = cn;
    u64 nip = cmd(mi, s->rn, s->rd);
    u64 mip = cmd(ni, s->rn, s->rd) - ni - nip;
    u64 tmp1 = cmd(ni, 2 * s->bn, s->bd);
    u64 tmp2 = cmd(ni, s->rn, s->rd) - ni + 110;
    u64 dn = umin(tmp1 + (u64)ceil((double)tmp2 / log2p), (u64)ceil((110.0 / (double)ni + s->dn1) / s->dn2));
    dn = umin(dn, mip);
    post[i][0] = nip; post[i][1] = mip; post[i][2] = dn;
  }
  return cnt;
}
/* matgen.rs:114-188: (m x n) CSC, exactly d sorted distinct row indices per column */
static int cmp_u64(const void *a, const void *b) { u64 x = *(const u64 *)a, y = *(const u64 *)b; return x < y ? -1 : x > y; }
static void gen_code(const fld_t *f, u64 n, u64 m, u64 d, lo_rng *g, csc_t *out) {
  const int L = f->L;
  out->rows = m; out->cols = n; out->nnz = n * d;
  out->colptr = malloc((n + 1) * 8);
  out->rowidx = malloc((n * d + 1) * 8);
  out->vals = malloc((n * d + 1) * L * 8);
  out->colptr[0] = 0;
  u64 k = 0;
  for (u64 c = 0; c < n; c++) {
    u64 *idx = out->rowidx + k;
    u64 got = 0;
    while (got < d) {
      u64 x = lo_rng_uniform(g, m);
      int dup = 0;
      for (u64 i = 0; i < got; i++) dup |= idx[i] == x;
      if (!dup) idx[got++] = x;
    }
    qsort(idx, d, 8, cmp_u64);
    for (u64 i = 0; i < d; i++) {
      u64 *v = out->vals + (k + i) * L;
      do rng_field_random1(g, f, v); while (fis_zero(v, L));
    }
    k += d;
    out->colptr[c + 1] = k;
  }
}
static u64 sdig_codeword_length(const csc_t *pre, const csc_t *post, int t) { /* encode.rs:18-33 */
  u64 s = pre[0].cols + post[t - 1].cols;
  for (int i = 0; i + 1 < t; i++) s += pre[i].rows;
  for (int i = 0; i < t; i++) s += post[i].rows;
  return s;
}
static u64 sdig_n_col_opens(int code) { /* brakedown lib.rs:57-61 */
  sdig_spec s;
  sdig_spec_get(code, &s);
  return (u64)ceil(-128.0 / log2(1.0 - s.dist / 3.0));
}
/* new (lib.rs:103-110) or, with ml != 0, new_ml (lib.rs:114-123), then _new_from_np1 (lib.rs:69-87) */
static int sdig_n_per_row_x(const fld_t *f, u64 len, int code, int ml, u64 *out) {
  u64 flog2 = f->num_bits - 1, n_col_opens = sdig_n_col_opens(code);
  double lncf = (double)(n_col_opens * len);
  double ndt = (double)n_degree_tests(128, (u64)ceil(sqrt(lncf)) * 2, flog2);
  u64 np1 = (u64)ceil(sqrt(lncf / ndt));
  if (ml) np1 = np2(np1);                               /* checked_next_power_of_two (lib.rs:119-121) */
  if (np1 > len) np1 = len;
  u64 nr1 = (len + np1 - 1) / np1, nd1 = n_degree_tests(128, np1 * 2, flog2);
  u64 np2_ = np1 / 2;
  if (np2_ == 0) return LO_ERR_ARG;
  u64 nr2 = (len + np2_ - 1) / np2_, nd2 = n_degree_tests(128, np2_ * 2, flog2);
  u64 sz1 = n_col_opens * nr1 + (1 + nd1) * np1, sz2 = n_col_opens * nr2 + (1 + nd2) * np2_;
  *out = sz1 < sz2 ? np1 : np2_;
  return 0;
}
static int sdig_n_per_row(const fld_t *f, u64 len, int code, u64 *out) { return sdig_n_per_row_x(f, len, code, 0, out); }
static int sdig_dims_x(int fid, u64 len, int code, int ml, u64 *nr, u64 *np, u64 *nc) {
  const fld_t *f = getf(fid);
  sdig_spec s;
  if (!f || sdig_spec_get(code, &s)) return LO_ERR_ARG;
  u64 npr;
  if (sdig_n_per_row_x(f, len, code, ml, &npr)) return LO_ERR_ARG;
  u64 pre[MAXLEV][3], post[MAXLEV][3];
  int t = sdig_get_dims(&s, npr, (double)(f->num_bits - 1), pre, post);
  if (t < 1) return LO_ERR_ARG;
  u64 c = pre[0][0] + post[t - 1][0];
  for (int i = 0; i + 1 < t; i++) c += pre[i][1];
  for (int i = 0; i < t; i++) c += post[i][1];
  *nr = (len + npr - 1) / npr; *np = npr; *nc = c;
  return 0;
}
int lo_sdig_get_dims(int fid, u64 len, int code, u64 *nr, u64 *np, u64 *nc) { return sdig_dims_x(fid, len, code, 0, nr, np, nc); }
/* SdigEncodingS::new_ml (lib.rs:114-123): dims for 2^n_vars monomials */
int lo_sdig_get_dims_ml(int fid, unsigned n_vars, int code, u64 *nr, u64 *np, u64 *nc) {
  if (n_vars >= 63) return LO_ERR_ARG;
  return sdig_dims_x(fid, (u64)1 << n_vars, code, 1, nr, np, nc);
}
/* LigeroEncodingRho::new_ml (ligero lib.rs:128-135): _get_dims + the three assert!s (LO_ERR_ARG when they fire) */
int lo_ligero_get_dims_ml(int fid, unsigned n_vars, unsigned rn, unsigned rd, u64 *nr, u64 *np, u64 *nc) {
  if (n_vars >= 63) return LO_ERR_ARG;
  u64 n = (u64)1 << n_vars;
  int rc = lo_ligero_get_dims(fid, n, rn, rd, nr, np, nc);
  if (rc) return rc;
  if ((*nr & (*nr - 1)) || (*np & (*np - 1)) || *nr * *np != n) return LO_ERR_ARG;
  return 0;
}
lo_enc *lo_sdig_new_from_dims(int fid, u64 n_per_row, u64 n_cols, u64 seed, int code) { /* lib.rs:126-137 + matgen.rs:28-52 */
  const fld_t *f = getf(fid);
  sdig_spec s;
  if (!f || sdig_spec_get(code, &s)) return NULL;
  u64 pre[MAXLEV][3], post[MAXLEV][3];
  int t = sdig_get_dims(&s, n_per_row, (double)(f->num_bits - 1), pre, post);
  if (t < 1) return NULL;
  lo_enc *e = calloc(1, sizeof *e);
  e->kind = LO_ENC_SDIG; e->fid = fid; e->f = f; e->n_per_row = n_per_row; e->code = code; e->seed = seed;
  e->n_levels = t;
  e->pre = calloc(t, sizeof(csc_t));
  e->post = calloc(t, sizeof(csc_t));
  for (int i = 0; i < t; i++) {
    lo_rng *g = lo_rng_seed_from_u64(seed);
    lo_rng_set_stream(g, (u64)i);
    gen_code(f, pre[i][0], pre[i][1], pre[i][2], g, &e->pre[i]);
    gen_code(f, post[i][0], post[i][1], post[i][2], g, &e->post[i]);
    lo_rng_free(g);
  }
  e->n_cols = sdig_codeword_length(e->pre, e->post, t);
  if (n_cols && n_cols != e->n_cols) { lo_enc_free(e); return NULL; }
  return e;
}
lo_enc *lo_sdig_new(int fid, u64 len, u64 seed, int code) {
  const fld_t *f = getf(fid);
  u64 npr;
  if (!f || sdig_n_per_row(f, len, code, &npr)) return NULL;
  return lo_sdig_new_from_dims(fid, npr, 0, seed, code);
}
void lo_enc_free(lo_enc *e) {
  if (!e) return;
  free(e->roots);
  for (int i = 0; i < e->n_levels; i++) {
    free(e->pre[i].colptr); free(e->pre[i].rowidx); free(e->pre[i].vals);
    free(e->post[i].colptr); free(e->post[i].rowidx); free(e->post[i].vals);
  }
  free(e->pre); free(e->post); free(e);
}
int lo_sdig_n_levels(const lo_enc *e) { return e->n_levels; }
int lo_sdig_matrix(const lo_enc *e, int level, int which, u64 *rows, u64 *cols, u64 *nnz,
                   const u64 **colptr, const u64 **rowidx, const u64 **vals) {
  if (e->kind != LO_ENC_SDIG || level < 0 || level >= e->n_levels) return LO_ERR_ARG;
  const csc_t *m = which ? &e->post[level] : &e->pre[level];
  *rows = m->rows; *cols = m->cols; *nnz = m->nnz; *colptr = m->colptr; *rowidx = m->rowidx; *vals = m->vals;
  return 0;
}
/* sprs CsMat::dot (CSC x dense) [3P]: out[i] += A[i,j] * x[j] */
AINL void csc_dot_L(const csc_t *A, const u64 *x, u64 *out, const fld_t *f, const int L) {
  memset(out, 0, A->rows * L * 8);
  for (u64 j = 0; j < A->cols; j++)
    for (u64 k = A->colptr[j]; k < A->colptr[j + 1]; k++) {
      u64 t[MAXL], *o = out + A->rowidx[k] * L;
      fmul(t, A->vals + k * L, x + j * L, f, L);
      fadd(o, o, t, f, L);
    }
}
static void csc_dot(const csc_t *A, const u64 *x, u64 *out, const fld_t *f) { DISPATCH_L(f, csc_dot_L(A, x, out, f, L)); }
static void sdig_encode(const lo_enc *e, u64 *xi) { /* encode.rs:36-110 */
  const fld_t *f = e->f;
  const int L = f->L, t = e->n_levels;
  u64 in_start = 0;
  for (int i = 0; i + 1 < t; i++) {
    u64 in_end = in_start + e->pre[i].cols;
    csc_dot(&e->pre[i], xi + in_start * L, xi + in_end * L, f);
    in_start = in_end;
  }
  const csc_t *pl = &e->pre[t - 1];
  u64 in_end = in_start + pl->cols;
  u64 *tmp = malloc((pl->rows + 1) * L * 8);
  csc_dot(pl, xi + in_start * L, tmp, f);
  u64 out_end = in_end + e->post[t - 1].cols;
  /* reed_solomon (encode.rs:97-110): Horner at points 1, 2, 3, ... */
  u64 x[MAXL], one[MAXL];
  fcopy(one, f->r, L);
  fcopy(x, f->r, L);
  for (u64 k = in_end; k < out_end; k++) {
    u64 r[MAXL] = { 0, 0, 0, 0 };
    for (u64 j = pl->rows; j-- > 0;) {
      DISPATCH_L(f, fmul(r, r, x, f, L); fadd(r, r, tmp + j * L, f, L));
    }
    fcopy(xi + k * L, r, L);
    DISPATCH_L(f, fadd(x, x, one, f, L));
  }
  free(tmp);
  in_start = in_end + pl->rows;
  u64 out_start = out_end;
  for (int i = t - 1; i >= 0; i--) {
    in_start -= e->pre[i].rows;
    csc_dot(&e->post[i], xi + in_start * L, xi + out_start * L, f);
    out_start += e->post[i].rows;
  }
}
void lo_enc_get_dims(const lo_enc *e, u64 len, u64 *nr, u64 *np, u64 *nc) {
  *nr = (len + e->n_per_row - 1) / e->n_per_row; *np = e->n_per_row; *nc = e->n_cols;
}
int lo_enc_dims_ok(const lo_enc *e, u64 n_per_row, u64 n_cols) {
  int ok = n_per_row < n_cols && n_per_row == e->n_per_row && n_cols == e->n_cols;
  if (e->kind == LO_ENC_LIGERO) ok = ok && (n_cols & (n_cols - 1)) == 0;
  return ok;
}
u64 lo_enc_n_col_opens(const lo_enc *e) {
  return e->kind == LO_ENC_LIGERO ? ligero_n_col_opens(e->rho_num, e->rho_den) : sdig_n_col_opens(e->code);
}
u64 lo_enc_n_degree_tests(const lo_enc *e) { return n_degree_tests(128, e->n_cols, e->f->num_bits - 1); }
int lo_enc_encode(const lo_enc *e, u64 *row) {
  if (e->kind == LO_ENC_LIGERO) fft_io_pc(e->f, row, e->n_cols, e->roots);
  else sdig_encode(e, row);
  return 0;
}

/* ======================================================================
 * LcCommit: lcpc-2d/src/lib.rs:172-184, 622-829
 * ====================================================================== */
struct lo_commit { const fld_t *f; u64 *comm, *coeffs; u64 n_rows, n_cols, n_per_row, n_hashes; u8 *hashes; };
#define LOG_MIN_NCOLS 5   /* lib.rs:619 */

AINL void hash_block_L(const lo_commit *c, u64 off, u64 cnt, const int L) {
  /* base case of hash_columns (lib.rs:716-735): <=32 streaming digests fed row by row */
  b3_t dig[1 << LOG_MIN_NCOLS];
  static const u8 zero[32] = { 0 };
  for (u64 i = 0; i < cnt; i++) { b3_init(&dig[i]); b3_update(&dig[i], zero, 32); }
  for (u64 row = 0; row < c->n_rows; row++)
    for (u64 col = 0; col < cnt; col++) {
      u64 t[MAXL];
      fcanon(t, c->comm + (row * c->n_cols + off + col) * L, c->f, L);   /* FieldHash::digest_update lib.rs:42-57 */
      b3_update(&dig[col], (const u8 *)t, 8 * L);
    }
  for (u64 i = 0; i < cnt; i++) b3_final(&dig[i], c->hashes + 32 * (off + i));
}
static void merkle_pair(const u8 *in, u8 *out) { lo_blake3(in, 64, out); } /* lib.rs:770-775 */
void lo_merkleize(lo_commit *c, int nthreads) {
  (void)nthreads;
  const u64 blk = 1 << LOG_MIN_NCOLS;
  const u64 nblk = (c->n_cols + blk - 1) / blk;
#pragma omp parallel for schedule(dynamic, 4) num_threads(nthreads > 0 ? nthreads : 1)
  for (u64 b = 0; b < nblk; b++) {
    u64 off = b * blk, cnt = umin(blk, c->n_cols - off);
    DISPATCH_L(c->f, hash_block_L(c, off, cnt, L));
  }
  u64 width = (c->n_hashes + 1) / 2, ins = 0, outs = width;
  while (width > 1) {
#pragma omp parallel for schedule(static) num_threads(nthreads > 0 ? nthreads : 1) if (width > 64)
    for (u64 i = 0; i < width / 2; i++) merkle_pair(c->hashes + 32 * (ins + 2 * i), c->hashes + 32 * (outs + i));
    ins = outs; outs += width / 2; width /= 2;
  }
}
void lo_hash_column(int fid, const u64 *col, u64 n_rows, u8 out[32]) {
  const fld_t *f = getf(fid);
  const int L = f->L;
  b3_t d;
  static const u8 zero[32] = { 0 };
  b3_init(&d);
  b3_update(&d, zero, 32);
  for (u64 r = 0; r < n_rows; r++) {
    u64 t[MAXL];
    DISPATCH_L(f, fcanon(t, col + r * L, f, L));
    b3_update(&d, (const u8 *)t, 8 * L);
  }
  b3_final(&d, out);
}
/* chunk CV of one column: chunk `ch` of the message 0^32 || repr(col[0]) || ... (bytes [1024 ch, 1024 ch + 1024)).
 * (_mt: columns spread over nthreads; the streaming whole-tree check of the full-size tests uses it.) */
int lo_leaf_chunk_cvs_mt(int fid, const u64 *comm, u64 n_cols, u64 row_base, u64 n_local, u64 n_rows, u64 cb, u64 ce, u8 *cvs, int nthreads) {
  const fld_t *f = getf(fid);
  if (!f) return LO_ERR_ARG;
  const int L = f->L;
  const u64 F = 8 * L, total = 32 + F * n_rows, n_chunks = (total + 1023) / 1024;
  int bad = 0;
#pragma omp parallel for schedule(static) num_threads(nthreads > 0 ? nthreads : 1) reduction(| : bad)
  for (u64 col = 0; col < n_cols; col++) {
    u8 msg[1024];
    for (u64 ch = cb; ch < ce && !bad; ch++) {
      const u64 off = ch * 1024, len = total - off < 1024 ? total - off : 1024;
      for (u64 b = 0; b < len;) {              /* assemble the chunk's bytes from the prefix and the local rows */
        const u64 pos = off + b;
        if (pos < 32) { msg[b++] = 0; continue; }
        const u64 row = (pos - 32) / F, within = (pos - 32) % F;
        if (row < row_base || row >= row_base + n_local) { bad = 1; break; }
        u64 t[MAXL];
        DISPATCH_L(f, fcanon(t, comm + ((row - row_base) * n_cols + col) * L, f, L));
        u64 take = F - within;
        if (take > len - b) take = len - b;
        memcpy(msg + b, (const u8 *)t + within, take);
        b += take;
      }
      if (bad) break;
      u32 cv[8];
      memcpy(cv, B3_IV, 32);
      const u64 nb = (len + 63) / 64;
      for (u64 b = 0; b < nb; b++) {
        u32 blk[16] = { 0 };
        const u64 bl = len - 64 * b < 64 ? len - 64 * b : 64;
        memcpy(blk, msg + 64 * b, bl);
        u32 flags = (b == 0 ? B3_CHUNK_START : 0) | (b == nb - 1 ? (B3_CHUNK_END | (n_chunks == 1 ? B3_ROOT : 0)) : 0);
        b3_compress(cv, blk, ch, (u32)bl, flags);
      }
      memcpy(cvs + ((ch - cb) * n_cols + col) * 32, cv, 32);
    }
  }
  return bad ? LO_ERR_ARG : 0;
}
int lo_leaf_chunk_cvs(int fid, const u64 *comm, u64 n_cols, u64 row_base, u64 n_local, u64 n_rows, u64 cb, u64 ce, u8 *cvs) {
  return lo_leaf_chunk_cvs_mt(fid, comm, n_cols, row_base, n_local, n_rows, cb, ce, cvs, 1);
}
static void b3_tree_from_cvs(const u32 (*cv)[8], u64 n, int is_root, u32 out[8]) {
  if (n == 1) { memcpy(out, cv[0], 32); return; }
  u64 left = 1;
  while (left * 2 < n) left *= 2;
  u32 blk[16];
  b3_tree_from_cvs(cv, left, 0, blk);
  b3_tree_from_cvs(cv + left, n - left, 0, blk + 8);
  memcpy(out, B3_IV, 32);
  b3_compress(out, blk, 0, 64, B3_PARENT | (is_root ? B3_ROOT : 0));
}
static void merkle_pair(const u8 *in, u8 *out);
int lo_finish_from_cvs_mt(const u8 *all, u64 n_chunks, u64 n_cols, u8 *hashes, int nthreads) {
  const u64 w0 = np2(n_cols);
  memset(hashes, 0, (2 * w0 - 1) * 32);
#pragma omp parallel num_threads(nthreads > 0 ? nthreads : 1)
  {
    u32 (*tmp)[8] = malloc(n_chunks * 32);
#pragma omp for schedule(static)
    for (u64 col = 0; col < n_cols; col++) {
      for (u64 ch = 0; ch < n_chunks; ch++) memcpy(tmp[ch], all + (ch * n_cols + col) * 32, 32);
      u32 out[8];
      b3_tree_from_cvs((const u32 (*)[8])tmp, n_chunks, 1, out);
      memcpy(hashes + 32 * col, out, 32);
    }
    free(tmp);
  }
  u64 width = w0, ins = 0, outs = w0;
  while (width > 1) {                           /* merkle_tree / merkle_layer, lib.rs:747-785 */
#pragma omp parallel for schedule(static) num_threads(nthreads > 0 ? nthreads : 1) if (width > 64)
    for (u64 i = 0; i < width / 2; i++) merkle_pair(hashes + 32 * (ins + 2 * i), hashes + 32 * (outs + i));
    ins = outs; outs += width / 2; width /= 2;
  }
  return 0;
}
int lo_finish_from_cvs(const u8 *all, u64 n_chunks, u64 n_cols, u8 *hashes) { return lo_finish_from_cvs_mt(all, n_chunks, n_cols, hashes, 1); }
/* the encode loop of commit alone (lib.rs:648-653): n_rows rows of n_per_row coefficients -> n_rows x n_cols, rows over threads */
int lo_encode_rows(const lo_enc *e, const u64 *coeffs, u64 n_rows, int nthreads, u64 *comm) {
  if (!e || !coeffs || !comm) return LO_ERR_ARG;
  const int L = e->f->L;
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads > 0 ? nthreads : 1)
  for (u64 r = 0; r < n_rows; r++) {
    u64 *row = comm + r * e->n_cols * L;
    memcpy(row, coeffs + r * e->n_per_row * L, e->n_per_row * L * 8);
    memset(row + e->n_per_row * L, 0, (e->n_cols - e->n_per_row) * L * 8);
    lo_enc_encode(e, row);
  }
  return 0;
}
void lo_merkleize_ser(lo_commit *c) { /* lib.rs:1127-1158 */
  const int L = c->f->L;
  u64 *col = malloc(c->n_rows * L * 8 + 8);
  for (u64 j = 0; j < c->n_cols; j++) {
    for (u64 r = 0; r < c->n_rows; r++) fcopy(col + r * L, c->comm + (r * c->n_cols + j) * L, L);
    int fid = (int)(c->f - FLD);
    lo_hash_column(fid, col, c->n_rows, c->hashes + 32 * j);
  }
  free(col);
  u64 width = (c->n_hashes + 1) / 2, ins = 0, outs = width;
  while (width > 1) {
    for (u64 i = 0; i < width / 2; i++) merkle_pair(c->hashes + 32 * (ins + 2 * i), c->hashes + 32 * (outs + i));
    ins = outs; outs += width / 2; width /= 2;
  }
}
/* zeroed buffer; large ones on 2 MiB-aligned, huge-page-advised memory: with 4 KiB pages a 256-thread first touch of the
 * multi-GB comm matrix spends seconds in the kernel's page-fault path, which is not the algorithm being timed */
static void *big_calloc(size_t bytes) {
  if (bytes < ((size_t)8 << 20)) return calloc(bytes ? bytes : 1, 1);
  void *p = NULL;
  const size_t rounded = (bytes + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
  if (posix_memalign(&p, (size_t)2 << 20, rounded)) return NULL;
#ifdef MADV_HUGEPAGE
  madvise(p, rounded, MADV_HUGEPAGE);
#endif
  const size_t n_chunks = rounded >> 21;
#pragma omp parallel for schedule(static)
  for (size_t i = 0; i < n_chunks; i++) memset((char *)p + (i << 21), 0, (size_t)1 << 21);
  return p;
}
static lo_commit *commit_alloc(const lo_enc *e, u64 n_rows) {
  lo_commit *c = calloc(1, sizeof *c);
  c->f = e->f; c->n_rows = n_rows; c->n_cols = e->n_cols; c->n_per_row = e->n_per_row;
  c->n_hashes = 2 * np2(e->n_cols) - 1;
  c->coeffs = big_calloc(n_rows * e->n_per_row * e->f->L * 8);
  c->comm = big_calloc(n_rows * e->n_cols * e->f->L * 8);
  c->hashes = big_calloc(c->n_hashes * 32);
  return c;
}
int lo_commit_new(const lo_enc *e, const u64 *coeffs_in, u64 n, int nthreads, lo_commit **out) { /* lib.rs:622-671 */
  if (!e || n == 0) return LO_ERR_ARG;
  const int L = e->f->L;
  u64 n_rows = (n + e->n_per_row - 1) / e->n_per_row;
  lo_commit *c = commit_alloc(e, n_rows);
  memcpy(c->coeffs, coeffs_in, n * L * 8);                          /* lib.rs:640-645 */
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads > 0 ? nthreads : 1)
  for (u64 r = 0; r < n_rows; r++) {                                /* lib.rs:648-653 */
    u64 *row = c->comm + r * c->n_cols * L;
    memcpy(row, c->coeffs + r * c->n_per_row * L, c->n_per_row * L * 8);
    lo_enc_encode(e, row);
  }
  lo_merkleize(c, nthreads);
  *out = c;
  return 0;
}
int lo_commit_from_parts(const lo_enc *e, const u64 *comm, const u64 *coeffs, u64 n_rows, lo_commit **out) {
  const int L = e->f->L;
  lo_commit *c = commit_alloc(e, n_rows);
  memcpy(c->comm, comm, n_rows * c->n_cols * L * 8);
  if (coeffs) memcpy(c->coeffs, coeffs, n_rows * c->n_per_row * L * 8);
  *out = c;
  return 0;
}
void lo_commit_free(lo_commit *c) { if (c) { free(c->comm); free(c->coeffs); free(c->hashes); free(c); } }
void lo_commit_dims(const lo_commit *c, u64 *nr, u64 *np, u64 *nc, u64 *nh) { *nr = c->n_rows; *np = c->n_per_row; *nc = c->n_cols; *nh = c->n_hashes; }
const u64 *lo_commit_comm(const lo_commit *c) { return c->comm; }
const u64 *lo_commit_coeffs(const lo_commit *c) { return c->coeffs; }
const u8 *lo_commit_hashes(const lo_commit *c) { return c->hashes; }
void lo_commit_root(const lo_commit *c, u8 out[32]) { memcpy(out, c->hashes + 32 * (c->n_hashes - 1), 32); } /* lib.rs:276-281 */

AINL void collapse_block_L(const lo_commit *c, const u64 *tensor, u64 *poly, u64 off, u64 cnt, const int L) {
  /* base case lib.rs:1105-1113 */
  for (u64 j = 0; j < cnt; j++) for (int k = 0; k < L; k++) poly[(off + j) * L + k] = 0;
  for (u64 row = 0; row < c->n_rows; row++)
    for (u64 j = 0; j < cnt; j++) {
      u64 t[MAXL], *o = poly + (off + j) * L;
      fmul(t, c->coeffs + (row * c->n_per_row + off + j) * L, tensor + row * L, c->f, L);
      fadd(o, o, t, c->f, L);
    }
}
int lo_collapse_columns(const lo_commit *c, const u64 *tensor, u64 n_tensor, u64 *poly, int nthreads) { /* lib.rs:1095-1123 */
  if (n_tensor != c->n_rows) return LO_ERR_OUTER_TENSOR;
  const u64 blk = 1 << LOG_MIN_NCOLS, nblk = (c->n_per_row + blk - 1) / blk;
#pragma omp parallel for schedule(dynamic, 4) num_threads(nthreads > 0 ? nthreads : 1)
  for (u64 b = 0; b < nblk; b++) {
    u64 off = b * blk, cnt = umin(blk, c->n_per_row - off);
    DISPATCH_L(c->f, collapse_block_L(c, tensor, poly, off, cnt, L));
  }
  return 0;
}
int lo_open_column(const lo_commit *c, u64 column, u64 *col_out, u8 *path_out) { /* lib.rs:788-825 */
  if (column >= c->n_cols) return LO_ERR_COLUMN_NUMBER;
  const int L = c->f->L;
  for (u64 r = 0; r < c->n_rows; r++) fcopy(col_out + r * L, c->comm + (r * c->n_cols + column) * L, L);
  u64 base = 0, width = (c->n_hashes + 1) / 2, plen = log2c(c->n_cols);
  for (u64 i = 0; i < plen; i++) {
    memcpy(path_out + 32 * i, c->hashes + 32 * (base + (column ^ 1)), 32);
    base += width; width /= 2; column >>= 1;
  }
  return 0;
}

/* ======================================================================
 * prove / verify: lib.rs:1004-1093, 832-1000; bincode layout lib.rs:186-609
 * ====================================================================== */
static const u8 LBL_DT[] = "$l//DT", LBL_PR[] = "$l//PR", LBL_PE[] = "$l//PE", LBL_CO[] = "$l//CO"; /* macros.rs:31-34 */
typedef struct { u8 *p; u64 len, cap; } wbuf;
static void wb_put(wbuf *w, const void *d, u64 n) {
  if (w->len + n > w->cap) { w->cap = (w->len + n) * 2 + 64; w->p = realloc(w->p, w->cap); }
  memcpy(w->p + w->len, d, n);
  w->len += n;
}
static void wb_u64(wbuf *w, u64 v) { wb_put(w, &v, 8); }
static void tr_absorb_poly(lo_transcript *tr, const u8 *label, const u64 *poly, u64 n, const fld_t *f) {
  const int L = f->L;
  for (u64 i = 0; i < n; i++) {
    u64 t[MAXL];
    DISPATCH_L(f, fcanon(t, poly + i * L, f, L));
    lo_tr_append_message(tr, label, 6, (const u8 *)t, 8 * L);     /* transcript_update lib.rs:47-49 */
  }
}
int lo_prove(const lo_commit *c, const lo_enc *e, const u64 *outer, u64 n_outer, lo_transcript *tr,
             u8 **proof, u64 *proof_len, u64 *cols_opened) {
  const fld_t *f = c->f;
  const int L = f->L;
  if (!lo_enc_dims_ok(e, c->n_per_row, c->n_cols)) return LO_ERR_COMMIT;
  if (n_outer != c->n_rows) return LO_ERR_OUTER_TENSOR;
  int fid = (int)(f - FLD);
  wbuf w = { 0, 0, 0 };
  u64 n_deg = lo_enc_n_degree_tests(e), n_open = lo_enc_n_col_opens(e), plen = log2c(c->n_cols);
  u64 *rand_tensor = malloc(c->n_rows * L * 8), *poly = malloc(c->n_per_row * L * 8);
  wbuf pr = { 0, 0, 0 };
  for (u64 i = 0; i < n_deg; i++) {                                   /* lib.rs:1024-1050 */
    u8 key[32];
    lo_tr_challenge_bytes(tr, LBL_DT, 6, key, 32);
    lo_rng *g = lo_rng_from_seed(key);
    lo_rng_field_random(g, fid, rand_tensor, c->n_rows);
    lo_rng_free(g);
    lo_collapse_columns(c, rand_tensor, c->n_rows, poly, 1);
    tr_absorb_poly(tr, LBL_PR, poly, c->n_per_row, f);
    wb_u64(&pr, c->n_per_row);
    wb_put(&pr, poly, c->n_per_row * L * 8);
  }
  lo_collapse_columns(c, outer, n_outer, poly, 1);                    /* lib.rs:1053-1068 */
  tr_absorb_poly(tr, LBL_PE, poly, c->n_per_row, f);
  /* bincode: n_cols, p_eval, p_random_vec, columns (WrappedLcEvalProof lib.rs:551-560) */
  wb_u64(&w, c->n_cols);
  wb_u64(&w, c->n_per_row);
  wb_put(&w, poly, c->n_per_row * L * 8);
  wb_u64(&w, n_deg);
  wb_put(&w, pr.p, pr.len);
  free(pr.p);
  u8 key[32];
  lo_tr_challenge_bytes(tr, LBL_CO, 6, key, 32);                      /* lib.rs:1071-1080 */
  lo_rng *g = lo_rng_from_seed(key);
  wb_u64(&w, n_open);
  u64 *col = malloc(c->n_rows * L * 8 + 8);
  u8 *path = malloc(32 * plen + 32);
  for (u64 i = 0; i < n_open; i++) {
    u64 cn = lo_rng_uniform(g, c->n_cols);
    if (cols_opened) cols_opened[i] = cn;
    lo_open_column(c, cn, col, path);
    wb_u64(&w, c->n_rows);
    wb_put(&w, col, c->n_rows * L * 8);
    wb_u64(&w, plen);
    for (u64 k = 0; k < plen; k++) { wb_u64(&w, 32); wb_put(&w, path + 32 * k, 32); }
  }
  lo_rng_free(g);
  free(col); free(path); free(rand_tensor); free(poly);
  *proof = w.p; *proof_len = w.len;
  return 0;
}
typedef struct { const u8 *p; u64 len, pos; int bad; } rbuf;
static u64 rb_u64(rbuf *r) { u64 v = 0; if (r->pos + 8 > r->len) { r->bad = 1; return 0; } memcpy(&v, r->p + r->pos, 8); r->pos += 8; return v; }
static const u8 *rb_take(rbuf *r, u64 n) { if (n > r->len - r->pos) { r->bad = 1; return NULL; } const u8 *q = r->p + r->pos; r->pos += n; return q; }
int lo_verify(const lo_enc *e, const u8 root[32], const u64 *outer, u64 n_outer, const u64 *inner, u64 n_inner,
              const u8 *proof, u64 proof_len, lo_transcript *tr, u64 *eval_out) {
  const fld_t *f = e->f;
  const int L = f->L;
  const u64 F = 8 * L;
  int fid = (int)(f - FLD);
  rbuf r = { proof, proof_len, 0, 0 };
  u64 n_cols = rb_u64(&r);
  u64 n_per_row = rb_u64(&r);
  if (r.bad || n_per_row > proof_len / F) return LO_VERR_MALFORMED;
  const u64 *p_eval = (const u64 *)rb_take(&r, n_per_row * F);
  u64 n_deg_pf = rb_u64(&r);
  if (r.bad || n_deg_pf > 1024) return LO_VERR_MALFORMED;
  const u64 **p_random = calloc(n_deg_pf + 1, sizeof(u64 *));
  for (u64 i = 0; i < n_deg_pf; i++) {
    u64 l = rb_u64(&r);
    if (r.bad || l != n_per_row) { free(p_random); return LO_VERR_MALFORMED; }
    p_random[i] = (const u64 *)rb_take(&r, l * F);
  }
  u64 n_columns = rb_u64(&r);
  if (r.bad) { free(p_random); return LO_VERR_MALFORMED; }
  int rc = 0;
  u64 n_col_opens = lo_enc_n_col_opens(e);                            /* lib.rs:845-848 */
  if (n_col_opens != n_columns || n_col_opens == 0) { free(p_random); return LO_VERR_NUM_COL_OPENS; }
  const u64 **cols = calloc(n_columns, sizeof(u64 *));
  const u8 **paths = calloc(n_columns, sizeof(u8 *));
  u64 *plens = calloc(n_columns, 8), n_rows = 0;
  for (u64 i = 0; i < n_columns && !r.bad; i++) {
    u64 l = rb_u64(&r);
    if (i == 0) n_rows = l;
    if (r.bad || l != n_rows || l > proof_len / F) { r.bad = 1; break; }
    cols[i] = (const u64 *)rb_take(&r, l * F);
    plens[i] = rb_u64(&r);
    if (r.bad || plens[i] > 64) { r.bad = 1; break; }
    paths[i] = r.p + r.pos;
    for (u64 k = 0; k < plens[i]; k++) { if (rb_u64(&r) != 32) r.bad = 1; rb_take(&r, 32); }
  }
  u64 *rand_tensors = NULL, *enc_rows = NULL;
  if (r.bad) { rc = LO_VERR_MALFORMED; goto done; }
  if (n_inner != n_per_row) { rc = LO_VERR_INNER_TENSOR; goto done; }   /* lib.rs:852-860 */
  if (n_outer != n_rows) { rc = LO_VERR_OUTER_TENSOR; goto done; }
  if (!lo_enc_dims_ok(e, n_per_row, n_cols)) { rc = LO_VERR_ENCODING_DIMS; goto done; }
  u64 n_deg = lo_enc_n_degree_tests(e);
  if (n_deg_pf < n_deg) { rc = LO_VERR_MALFORMED; goto done; }           /* reference would panic indexing p_random_vec[i] */
  rand_tensors = malloc((n_deg + 1) * n_rows * F);
  enc_rows = calloc((n_deg + 1) * n_cols, F);
  for (u64 i = 0; i < n_deg; i++) {                                   /* lib.rs:868-894 */
    u8 key[32];
    lo_tr_challenge_bytes(tr, LBL_DT, 6, key, 32);
    lo_rng *g = lo_rng_from_seed(key);
    lo_rng_field_random(g, fid, rand_tensors + i * n_rows * L, n_rows);
    lo_rng_free(g);
    memcpy(enc_rows + i * n_cols * L, p_random[i], n_per_row * F);
    lo_enc_encode(e, enc_rows + i * n_cols * L);
    tr_absorb_poly(tr, LBL_PR, p_random[i], n_per_row, f);
  }
  tr_absorb_poly(tr, LBL_PE, p_eval, n_per_row, f);                   /* lib.rs:896-899 */
  u8 key[32];
  lo_tr_challenge_bytes(tr, LBL_CO, 6, key, 32);                      /* lib.rs:902-911 */
  lo_rng *g = lo_rng_from_seed(key);
  u64 *p_eval_fft = enc_rows + n_deg * n_cols * L;
  memcpy(p_eval_fft, p_eval, n_per_row * F);                          /* lib.rs:914-920 */
  lo_enc_encode(e, p_eval_fft);
  for (u64 i = 0; i < n_columns && rc == 0; i++) {                    /* lib.rs:923-944 */
    u64 cn = lo_rng_uniform(g, n_cols);
    int rnd = 1, evl, pth;
    for (u64 d = 0; d <= n_deg; d++) {
      const u64 *tensor = d < n_deg ? rand_tensors + d * n_rows * L : outer;
      u64 acc[MAXL] = { 0, 0, 0, 0 }, t[MAXL];
      for (u64 k = 0; k < n_rows; k++) { DISPATCH_L(f, fmul(t, tensor + k * L, cols[i] + k * L, f, L); fadd(acc, acc, t, f, L)); }
      int ok = feq(acc, enc_rows + (d * n_cols + cn) * L, L);          /* verify_column_value lib.rs:985-1000 */
      if (d < n_deg) rnd &= ok; else evl = ok;
    }
    u8 h[32], blk[64];                                                /* verify_column_path lib.rs:955-982 */
    lo_hash_column(fid, cols[i], n_rows, h);
    u64 cc = cn;
    for (u64 k = 0; k < plens[i]; k++) {
      const u8 *pk = paths[i] + 40 * k + 8;
      if (cc % 2 == 0) { memcpy(blk, h, 32); memcpy(blk + 32, pk, 32); } else { memcpy(blk, pk, 32); memcpy(blk + 32, h, 32); }
      lo_blake3(blk, 64, h);
      cc >>= 1;
    }
    pth = memcmp(h, root, 32) == 0;
    if (!rnd) rc = LO_VERR_COLUMN_DEGREE; else if (!evl) rc = LO_VERR_COLUMN_EVAL; else if (!pth) rc = LO_VERR_COLUMN_PATH;
  }
  lo_rng_free(g);
  if (rc == 0) {                                                      /* lib.rs:947-951 */
    u64 acc[MAXL] = { 0, 0, 0, 0 }, t[MAXL];
    for (u64 k = 0; k < n_per_row; k++) { DISPATCH_L(f, fmul(t, inner + k * L, p_eval + k * L, f, L); fadd(acc, acc, t, f, L)); }
    fcopy(eval_out, acc, L);
  }
done:
  free(rand_tensors); free(enc_rows); free(cols); free(paths); free(plens); free(p_random);
  return rc;
}
void lo_free(void *p) { free(p); }
