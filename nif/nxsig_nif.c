/*
 * nxsig_nif.c — dirty-NIF shim between the BEAM and the C ABI in include/nxsig.h.
 *
 * The build image has no Erlang/OTP (no erl, no erl_nif.h), so nif/Makefile builds this file only where `erl` is
 * found.  It is nevertheless compiled and EXECUTED by the test-suite: tests/stub/erl_nif.h declares the subset of the NIF
 * API used here and tests/stub/erl_nif_fake.c is a miniature term runtime, so tests/test_nif_shim.py (CPU: host generators,
 * argument validation; GPU: stft / istft / fir / device chains / sharded calls) calls these functions exactly as the BEAM
 * would (entry->funcs[i].fptr(env, argc, argv)) and compares with the ctypes path bit for bit; tests/test_nif_calls_host.py
 * pins what every NIF hands to the C ABI and gives back, error paths included, against a recording stand-in for the library.
 *
 * The shim is deliberately mechanical: every function unpacks terms, validates sizes BEFORE allocating, calls ONE
 * nxsig_* entry point and packs the result; all logic lives behind the C ABI.
 *
 * A new NIF is written with three helpers.  get_rows() reads a tensor operand — a binary of EXACTLY elem * a * b * c bytes, or a
 * device buffer of the call's context that holds at least as many.  result_t holds the result — a BEAM binary or a device block —
 * behind res_open() / res_fail() / res_term(), so that a NIF has one error exit whatever it allocated.  get_frames_args() is the
 * argument prologue of the STFT family (length or frame count, batch, window, [window_is_f64,] params, the window size check and
 * the rows' output length).  Where two table entries differ only in an element type (f32 / f64, c64 / c128) or in where the tensors
 * live (host / device), they are one body with that as a parameter and the callee chosen by a branch at the single call site.
 *
 * Conventions:
 *   - every GPU call is a dirty job (ERL_NIF_DIRTY_JOB_IO_BOUND: the scheduler thread waits on the GPU);
 *   - inputs are borrowed binaries (enif_inspect_binary, read-only, valid for the call); host outputs are BEAM-owned
 *     binaries (enif_alloc_binary, which can FAIL without taking the VM down, then enif_make_binary); device tensors are
 *     resource objects whose destructor frees HBM;
 *   - errors come back as {:error, {code, message}} (code -1 = ArgumentError on the Elixir side); malformed terms are
 *     badarg; nothing throws, aborts or longjmps across the boundary;
 *   - a context resource owns one GPU + one HIP stream; libnxsig serialises calls per context internally, so dirty
 *     schedulers may call concurrently from any OS thread;
 *   - a group resource owns one context per member GPU and the RCCL communicators (nxsig_group_create_local).
 */
#include <erl_nif.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../include/nxsig.h"

/* What this file assumes about <erl_nif.h>, checked at COMPILE time against whichever header it meets — the stand-in of the test
 * suite (tests/stub/erl_nif.h, written from the documentation) or a real OTP one (nif/Makefile, -Werror).  A first `mix compile`
 * on a BEAM box that disagrees with any of these stops here with the reason, not in a dirty scheduler at run time. */
_Static_assert(sizeof(ERL_NIF_TERM) == sizeof(void*), "ERL_NIF_TERM is one machine word");
_Static_assert(sizeof(ErlNifSInt64) == 8 && sizeof(ErlNifUInt64) == 8, "64-bit integer terms (enif_get_int64 / enif_make_int64)");
_Static_assert(ERL_NIF_DIRTY_JOB_CPU_BOUND == 1 && ERL_NIF_DIRTY_JOB_IO_BOUND == 2, "dirty-scheduler flags of ErlNifFunc.flags");
_Static_assert(offsetof(ErlNifBinary, size) == 0 && offsetof(ErlNifBinary, data) == sizeof(size_t), "ErlNifBinary starts {size, data}");
_Static_assert(offsetof(ErlNifFunc, name) == 0 && offsetof(ErlNifFunc, arity) == sizeof(char*) &&
               offsetof(ErlNifFunc, fptr) > offsetof(ErlNifFunc, arity) && offsetof(ErlNifFunc, flags) > offsetof(ErlNifFunc, fptr),
               "ErlNifFunc is {name, arity, fptr, flags}: the funcs[] table below is written positionally");
_Static_assert(offsetof(ErlNifEntry, major) == 0 && offsetof(ErlNifEntry, funcs) > offsetof(ErlNifEntry, num_of_funcs),
               "ErlNifEntry starts {major, minor, name, num_of_funcs, funcs}");
_Static_assert(ERL_NIF_RT_CREATE == 1 && ERL_NIF_RT_TAKEOVER == 2, "resource-type flags");
_Static_assert(ERL_NIF_LATIN1 == 1, "atom encoding passed to enif_get_atom");
#ifdef ERL_NIF_MAJOR_VERSION   /* a real OTP header: dirty NIFs without a build flag need NIF API 2.11 (OTP 20) or later */
_Static_assert(ERL_NIF_MAJOR_VERSION == 2 && ERL_NIF_MINOR_VERSION >= 11, "needs the NIF API of OTP 20 or later (dirty schedulers)");
#endif
_Static_assert(sizeof(nxsig_c64) == 8 && sizeof(float) == 4 && sizeof(double) == 8, "tensor element sizes of the binaries");

static ErlNifResourceType* CTX_RES;
static ErlNifResourceType* BUF_RES;
static ErlNifResourceType* GRP_RES;

typedef struct { nxsig_ctx* ctx; } ctx_res_t;
typedef struct { nxsig_group* grp; } grp_res_t;
/* a device buffer lives on ONE context: a context resource (owner) or member `member` of a group (gowner); the buffer keeps
 * whichever it belongs to alive, so the memory can always be returned to the allocator it came from */
typedef struct { ctx_res_t* owner; grp_res_t* gowner; int member; void* dptr; size_t bytes; } buf_res_t;

static void ctx_dtor(ErlNifEnv* env, void* obj) { (void)env; ctx_res_t* r = obj; if (r->ctx) nxsig_ctx_destroy(r->ctx); }
static void buf_dtor(ErlNifEnv* env, void* obj) {
  (void)env;
  buf_res_t* b = obj;
  if (b->dptr && b->owner && b->owner->ctx) nxsig_free(b->owner->ctx, b->dptr);
  if (b->dptr && b->gowner && b->gowner->grp) {
    nxsig_ctx* c = nxsig_group_ctx(b->gowner->grp, b->member);
    if (c) nxsig_free(c, b->dptr);
  }
  if (b->owner) enif_release_resource(b->owner);
  if (b->gowner) enif_release_resource(b->gowner);
}
static nxsig_ctx* buf_ctx(const buf_res_t* b) {
  if (b->owner) return b->owner->ctx;
  if (b->gowner && b->gowner->grp) return nxsig_group_ctx(b->gowner->grp, b->member);
  return NULL;
}
static void grp_dtor(ErlNifEnv* env, void* obj) { (void)env; grp_res_t* g = obj; if (g->grp) nxsig_group_destroy(g->grp); }

static ERL_NIF_TERM mk_atom(ErlNifEnv* env, const char* a) { return enif_make_atom(env, a); }
static ERL_NIF_TERM mk_error_msg(ErlNifEnv* env, int code, const char* msg) {
  ErlNifBinary b;
  size_t n = msg ? strlen(msg) : 0;
  ERL_NIF_TERM m;
  if (enif_alloc_binary(n, &b)) { if (n) memcpy(b.data, msg, n); m = enif_make_binary(env, &b); }
  else m = mk_atom(env, "enomem");
  return enif_make_tuple2(env, mk_atom(env, "error"), enif_make_tuple2(env, enif_make_int(env, code), m));
}
static ERL_NIF_TERM mk_error(ErlNifEnv* env, int code) { return mk_error_msg(env, code, nxsig_last_error()); }
static ERL_NIF_TERM mk_oom(ErlNifEnv* env) { return mk_error_msg(env, NXSIG_ERR_OOM, "cannot allocate the result binary"); }
static ERL_NIF_TERM mk_ok(ErlNifEnv* env, ERL_NIF_TERM v) { return enif_make_tuple2(env, mk_atom(env, "ok"), v); }
static ERL_NIF_TERM mk_ok2(ErlNifEnv* env, ERL_NIF_TERM v, ERL_NIF_TERM w) { return enif_make_tuple3(env, mk_atom(env, "ok"), v, w); }

/* sizes are overflow-checked */
static int mul_size(size_t* acc, uint64_t f) {
  if (f != 0 && *acc > (size_t)-1 / f) return 0;
  *acc *= (size_t)f;
  return 1;
}
static int rows_bytes(size_t* n, size_t elem, uint64_t a, uint64_t b, uint64_t c) {
  *n = elem;
  return mul_size(n, a) && mul_size(n, b) && mul_size(n, c);
}

static int get_ctx(ErlNifEnv* env, ERL_NIF_TERM t, ctx_res_t** out) {
  return enif_get_resource(env, t, CTX_RES, (void**)out) && (*out)->ctx != NULL;
}
static int get_buf(ErlNifEnv* env, ERL_NIF_TERM t, buf_res_t** out) { return enif_get_resource(env, t, BUF_RES, (void**)out); }
static int get_grp(ErlNifEnv* env, ERL_NIF_TERM t, grp_res_t** out) {
  return enif_get_resource(env, t, GRP_RES, (void**)out) && (*out)->grp != NULL;
}
/* Elixir numbers arrive as floats or integers */
static int get_number(ErlNifEnv* env, ERL_NIF_TERM t, double* d) {
  ErlNifSInt64 i;
  if (enif_get_double(env, t, d)) return 1;
  if (enif_get_int64(env, t, &i)) { *d = (double)i; return 1; }
  return 0;
}

/* {n, hop, k, pad_mode, pad_lo, pad_hi, scaling, sampling_rate} -> nxsig_stft_params; geometry is validated here so that
 * no size below is computed from a non-positive length (a negative fft_length reached enif_make_new_binary) */
static int get_params(ErlNifEnv* env, ERL_NIF_TERM t, nxsig_stft_params* p) {
  const ERL_NIF_TERM* e;
  int arity;
  ErlNifSInt64 lo, hi;
  int n, hop, k, pad, scal;
  double fs;
  if (!enif_get_tuple(env, t, &arity, &e) || arity != 8) return 0;
  if (!enif_get_int(env, e[0], &n) || !enif_get_int(env, e[1], &hop) || !enif_get_int(env, e[2], &k) ||
      !enif_get_int(env, e[3], &pad) || !enif_get_int64(env, e[4], &lo) || !enif_get_int64(env, e[5], &hi) ||
      !enif_get_int(env, e[6], &scal) || !get_number(env, e[7], &fs))
    return 0;
  if (n < 1 || k < 1) return 0;
  memset(p, 0, sizeof *p);
  p->frame_length = n; p->hop = hop; p->fft_length = k; p->pad_mode = pad; p->pad_lo = lo; p->pad_hi = hi;
  p->scaling = scal; p->sampling_rate = fs;
  return 1;
}

static ERL_NIF_TERM make_buf(ErlNifEnv* env, ctx_res_t* c, void* d, size_t bytes) {
  buf_res_t* r = enif_alloc_resource(BUF_RES, sizeof *r);
  r->owner = c; enif_keep_resource(c); r->gowner = NULL; r->member = 0; r->dptr = d; r->bytes = bytes;
  ERL_NIF_TERM t = enif_make_resource(env, r);
  enif_release_resource(r);
  return t;
}
/* a buffer on member `member` of a group */
static ERL_NIF_TERM make_gbuf(ErlNifEnv* env, grp_res_t* g, int member, void* d, size_t bytes) {
  buf_res_t* r = enif_alloc_resource(BUF_RES, sizeof *r);
  r->owner = NULL; r->gowner = g; enif_keep_resource(g); r->member = member; r->dptr = d; r->bytes = bytes;
  ERL_NIF_TERM t = enif_make_resource(env, r);
  enif_release_resource(r);
  return t;
}

/* ------------------------------------------------------------------------------------------------ operands and results */
/* A tensor operand: a x b x c items of `elem` bytes, every count at least 1.  mem NXSIG_HOST: a binary of exactly that many bytes — the
 * library reads all of them and not one more, so neither a short binary nor one with trailing elements is let through.  NXSIG_DEVICE: a
 * buffer resource that lives on context c and holds at least that many bytes (a buffer may be larger than the tensor it carries). */
static int get_rows(ErlNifEnv* env, ERL_NIF_TERM t, const ctx_res_t* c, int mem, size_t elem, int64_t a, int64_t b, int64_t d, const void** data) {
  size_t need;
  if (a < 1 || b < 1 || d < 1 || !rows_bytes(&need, elem, (uint64_t)a, (uint64_t)b, (uint64_t)d)) return 0;
  if (mem == NXSIG_HOST) {
    ErlNifBinary bin;
    if (!enif_inspect_binary(env, t, &bin) || bin.size != need) return 0;
    *data = bin.data;
  } else {
    buf_res_t* buf;
    if (!get_buf(env, t, &buf) || buf->owner != c || buf->bytes < need) return 0;
    *data = buf->dptr;
  }
  return 1;
}

/* A result tensor: a BEAM binary (NXSIG_HOST; enif_alloc_binary reports failure instead of aborting the VM) or a block of context c's
 * device memory (NXSIG_DEVICE).  res_open returns 0, RES_NOMEM or the library's (negative) status; res_fail releases whatever n results
 * hold and makes the error term; res_term hands the tensor to the BEAM as a binary or a buffer resource. */
typedef struct { int open, mem; ctx_res_t* c; ErlNifBinary bin; void* data; size_t bytes; } result_t;
enum { RES_NOMEM = 1 };

static int res_open(result_t* r, ctx_res_t* c, int mem, size_t elem, uint64_t a, uint64_t b, uint64_t d) {
  if (!rows_bytes(&r->bytes, elem, a, b, d)) return RES_NOMEM;
  r->mem = mem; r->c = c;
  if (mem == NXSIG_HOST) {
    if (r->bytes > ((size_t)1 << 46)) return RES_NOMEM; /* 64 TiB: far beyond any host; keeps a bad shape from reaching the allocator */
    if (!enif_alloc_binary(r->bytes, &r->bin)) return RES_NOMEM;
    r->data = r->bin.data;
  } else {
    int rc = nxsig_alloc(c->ctx, r->bytes, &r->data);
    if (rc) return rc;
  }
  r->open = 1;
  return 0;
}
static ERL_NIF_TERM res_fail(ErlNifEnv* env, result_t* r, int n, int rc) {
  for (int i = 0; i < n; ++i) {
    if (r[i].open && r[i].mem == NXSIG_HOST) enif_release_binary(&r[i].bin);
    if (r[i].open && r[i].mem != NXSIG_HOST) nxsig_free(r[i].c->ctx, r[i].data);
    r[i].open = 0;
  }
  return rc == RES_NOMEM ? mk_oom(env) : mk_error(env, rc);
}
static ERL_NIF_TERM res_term(ErlNifEnv* env, result_t* r) {
  return r->mem == NXSIG_HOST ? enif_make_binary(env, &r->bin) : make_buf(env, r->c, r->data, r->bytes);
}
/* the usual ending: {:ok, result} or the error of status rc */
static ERL_NIF_TERM res_ok(ErlNifEnv* env, result_t* r, int rc) { return rc ? res_fail(env, r, 1, rc) : mk_ok(env, res_term(env, r)); }
/* ... and {:ok, result, count} */
static ERL_NIF_TERM res_ok2(ErlNifEnv* env, result_t* r, int rc, int64_t count) {
  return rc ? res_fail(env, r, 1, rc) : mk_ok2(env, res_term(env, r), enif_make_int64(env, count));
}
static int term_mem(ErlNifEnv* env, ERL_NIF_TERM t) {
  ErlNifBinary b;
  return enif_inspect_binary(env, t, &b) ? NXSIG_HOST : NXSIG_DEVICE;
}

/* The argument run every STFT-family NIF has at argv[2 ...]: length, batch, window_bin, [window_is_f64 — the f64 tier,] params; for the
 * inverse transforms the first is num_frames.  `out` is what the geometry makes of one row: nxsig_num_frames(length ...) frames, or for
 * the inverse nxsig_ola_length(num_frames ...) samples; negative: the library's status, to be reported with mk_error once the NIF's
 * remaining arguments have passed their own checks (badarg comes first). */
typedef struct {
  ErlNifSInt64 len;
  int batch, wf64;
  ErlNifBinary w;
  nxsig_stft_params p;
  int64_t out;
} frames_args_t;
static int get_frames_args(ErlNifEnv* env, const ERL_NIF_TERM* argv, int wide, int inverse, frames_args_t* a) {
  a->wf64 = 0;
  if (!enif_get_int64(env, argv[0], &a->len) || !enif_get_int(env, argv[1], &a->batch) || !enif_inspect_binary(env, argv[2], &a->w) ||
      (wide && !enif_get_int(env, argv[3], &a->wf64)) || !get_params(env, argv[wide ? 4 : 3], &a->p))
    return 0;
  /* the window binary is read by the library: its size must match (a short window was read out of bounds) */
  if (a->batch < 1 || a->len < 1 || a->w.size != (size_t)a->p.frame_length * (a->wf64 ? 8 : 4)) return 0;
  a->out = inverse ? nxsig_ola_length(a->len, a->p.frame_length, a->p.hop)
                   : nxsig_num_frames(a->len, a->p.frame_length, a->p.hop, a->p.pad_mode, a->p.pad_lo, a->p.pad_hi);
  return 1;
}

/* ------------------------------------------------------------------------------------------------ contexts */
static ERL_NIF_TERM nif_device_count(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  (void)argv;
  int n = 0;
  if (argc != 0) return enif_make_badarg(env);
  int rc = nxsig_device_count(&n);
  return rc ? mk_error(env, rc) : mk_ok(env, enif_make_int(env, n));
}

static ERL_NIF_TERM nif_ctx_create(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  int dev;
  if (argc != 1 || !enif_get_int(env, argv[0], &dev)) return enif_make_badarg(env);
  nxsig_ctx* c = NULL;
  int rc = nxsig_ctx_create(dev, &c);
  if (rc) return mk_error(env, rc);
  ctx_res_t* r = enif_alloc_resource(CTX_RES, sizeof *r);
  r->ctx = c;
  ERL_NIF_TERM t = enif_make_resource(env, r);
  enif_release_resource(r);
  return mk_ok(env, t);
}

static ERL_NIF_TERM nif_sync(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  if (argc != 1 || !get_ctx(env, argv[0], &c)) return enif_make_badarg(env);
  int rc = nxsig_sync(c->ctx);
  return rc ? mk_error(env, rc) : mk_atom(env, "ok");
}

/* last_dispatch(ctx) -> {:ok, binary}: the kernel families of the last compute call on this context ("stft.pair", "istft.wave.deep+
 * istft.edge_chunks" ...; include/nxsig.h: nxsig_ctx_last_dispatch — the per-context copy, because two NIF calls of one Erlang process
 * may run on different scheduler threads).  Diagnostic: NxSignalAMD.last_dispatch/1 */
static ERL_NIF_TERM nif_last_dispatch(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  if (argc != 1 || !get_ctx(env, argv[0], &c)) return enif_make_badarg(env);
  char buf[512];
  int rc = nxsig_ctx_last_dispatch(c->ctx, buf, sizeof buf);
  if (rc) return mk_error(env, rc);
  ErlNifBinary b;
  const size_t n = strlen(buf);
  if (!enif_alloc_binary(n, &b)) return mk_oom(env);
  memcpy(b.data, buf, n);
  return mk_ok(env, enif_make_binary(env, &b));
}

/* ------------------------------------------------------------------------------------------------ host generators
 * The reference computes in the type of its operands (include/nxsig.h "f64 / c128 tier"): each generator has an _f64 entry that
 * takes the same terms and returns an f64 binary. */
/* window(kind, n, periodic, beta, eps) -> {:ok, f32 binary}   (NxSignal.Windows.*, BinaryBackend rounding)
 * window_f64: the same -> {:ok, f64 binary}   (NxSignal.Windows.*(n, type: {:f, 64})) */
static ERL_NIF_TERM window_any(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[], int f64) {
  int kind, n, per;
  double beta, eps;
  result_t o = {0};
  if (argc != 5 || !enif_get_int(env, argv[0], &kind) || !enif_get_int(env, argv[1], &n) || !enif_get_int(env, argv[2], &per) ||
      !get_number(env, argv[3], &beta) || !get_number(env, argv[4], &eps) || n < 0)
    return enif_make_badarg(env);
  int rc = res_open(&o, NULL, NXSIG_HOST, f64 ? 8 : 4, (uint64_t)n, 1, 1);
  if (!rc) rc = f64 ? nxsig_window_f64(kind, n, per, beta, eps, (double*)o.data) : nxsig_window_f32(kind, n, per, beta, eps, (float*)o.data);
  return res_ok(env, &o, rc);
}
static ERL_NIF_TERM nif_window(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return window_any(env, argc, argv, 0); }
static ERL_NIF_TERM nif_window_f64(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return window_any(env, argc, argv, 1); }

/* firwin(num_taps, [cutoff], window_kind, beta, pass_zero, scale, sampling_rate) -> {:ok, f32 binary}; firwin_f64 -> {:ok, f64 binary} */
static ERL_NIF_TERM firwin_any(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[], int f64) {
  int taps, kind, pz, sc;
  double beta, fs, cut[64];
  unsigned len;
  result_t o = {0};
  if (argc != 7 || !enif_get_int(env, argv[0], &taps) || !enif_get_list_length(env, argv[1], &len) || len > 64 ||
      !enif_get_int(env, argv[2], &kind) || !get_number(env, argv[3], &beta) || !enif_get_int(env, argv[4], &pz) ||
      !enif_get_int(env, argv[5], &sc) || !get_number(env, argv[6], &fs) || taps < 1)
    return enif_make_badarg(env);
  ERL_NIF_TERM head, tail = argv[1];
  for (unsigned i = 0; i < len; ++i)
    if (!enif_get_list_cell(env, tail, &head, &tail) || !get_number(env, head, &cut[i])) return enif_make_badarg(env);
  int rc = res_open(&o, NULL, NXSIG_HOST, f64 ? 8 : 4, (uint64_t)taps, 1, 1);
  if (!rc) rc = f64 ? nxsig_firwin_f64(taps, cut, (int)len, kind, beta, pz, sc, fs, (double*)o.data)
                    : nxsig_firwin_f32(taps, cut, (int)len, kind, beta, pz, sc, fs, (float*)o.data);
  return res_ok(env, &o, rc);
}
static ERL_NIF_TERM nif_firwin(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return firwin_any(env, argc, argv, 0); }
static ERL_NIF_TERM nif_firwin_f64(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return firwin_any(env, argc, argv, 1); }

/* fft_frequencies(sampling_rate, fft_length, endpoint) -> {:ok, f32 binary}   (lib/nx_signal.ex:154-166); fft_frequencies_f64 -> f64 */
static ERL_NIF_TERM fft_frequencies_any(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[], int f64) {
  double fs;
  int k, endpoint;
  result_t o = {0};
  if (argc != 3 || !get_number(env, argv[0], &fs) || !enif_get_int(env, argv[1], &k) || !enif_get_int(env, argv[2], &endpoint) || k < 1)
    return enif_make_badarg(env);
  int rc = res_open(&o, NULL, NXSIG_HOST, f64 ? 8 : 4, (uint64_t)k, 1, 1);
  if (!rc) rc = f64 ? nxsig_fft_frequencies_f64(fs, k, endpoint, (double*)o.data) : nxsig_fft_frequencies_f32(fs, k, endpoint, (float*)o.data);
  return res_ok(env, &o, rc);
}
static ERL_NIF_TERM nif_fft_frequencies(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return fft_frequencies_any(env, argc, argv, 0); }
static ERL_NIF_TERM nif_fft_frequencies_f64(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return fft_frequencies_any(env, argc, argv, 1); }

/* mel_filters(fft_length, mel_bins, sampling_rate, max_mel, mel_frequency_spacing) -> {:ok, f32[mel_bins][fft_length]} (:397-445) */
static ERL_NIF_TERM nif_mel_filters(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  int k, bins;
  double fs, max_mel, sp;
  result_t o = {0};
  if (argc != 5 || !enif_get_int(env, argv[0], &k) || !enif_get_int(env, argv[1], &bins) || !get_number(env, argv[2], &fs) ||
      !get_number(env, argv[3], &max_mel) || !get_number(env, argv[4], &sp) || k < 1 || bins < 1)
    return enif_make_badarg(env);
  int rc = res_open(&o, NULL, NXSIG_HOST, 4, (uint64_t)k, (uint64_t)bins, 1);
  if (!rc) rc = nxsig_mel_filters_f32(k, bins, fs, max_mel, sp, (float*)o.data);
  return res_ok(env, &o, rc);
}

/* sinc(t_bin) -> {:ok, f32 binary}   (lib/nx_signal/waveforms.ex:451-457); sinc_f64: f64 in, f64 out */
static ERL_NIF_TERM sinc_any(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[], int f64) {
  const size_t elem = f64 ? 8 : 4;
  ErlNifBinary t;
  result_t o = {0};
  if (argc != 1 || !enif_inspect_binary(env, argv[0], &t) || t.size % elem) return enif_make_badarg(env);
  const int64_t n = (int64_t)(t.size / elem);
  int rc = res_open(&o, NULL, NXSIG_HOST, elem, (uint64_t)n, 1, 1);
  if (!rc) rc = f64 ? nxsig_sinc_f64((const double*)t.data, n, (double*)o.data) : nxsig_sinc_f32((const float*)t.data, n, (float*)o.data);
  return res_ok(env, &o, rc);
}
static ERL_NIF_TERM nif_sinc(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return sinc_any(env, argc, argv, 0); }
static ERL_NIF_TERM nif_sinc_f64(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return sinc_any(env, argc, argv, 1); }

/* ------------------------------------------------------------------------------------------------ hot path
 * One body per call family.  `mem`: the tensors are binaries (NXSIG_HOST) or buffer resources of the context (NXSIG_DEVICE: the chain
 * stft -> edit -> istft stays in HBM; guides/filtering.livemd:137-159; device calls are asynchronous on the
 * context's stream, from_device synchronises).  `f64`: the f64 / c128 tier (include/nxsig.h), whose NIFs take window_is_f64 after the
 * window: f64 / c128 binaries in, the same out. */
/* stft(ctx, x_bin, length, batch, window_bin, params) -> {:ok, z_bin, num_frames, times_bin, freqs_bin}
 * stft_c64: the same with x_bin holding c64 samples (interleaved f32 re, im) — lib/nx_signal.ex:94-102 on complex data
 * stft_f64(ctx, x_bin (f64), length, batch, window_bin, window_is_f64, params) -> {:ok, z_bin (c128), num_frames, times_bin, freqs_bin}
 * stft_c128: the same with complex f64 samples (lib/nx_signal.ex:94-102 on a c128 tensor, or c64 samples under an f64 window);
 *   times / frequencies stay f32 like the reference's (lib/nx_signal.ex:106-111)
 * stft_dev(ctx, x_buf, length, batch, window_bin, params) -> {:ok, z_buf, num_frames}; stft_c64_dev: x_buf holds c64 samples */
static ERL_NIF_TERM stft_any(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[], int cplx, int f64, int mem) {
  ctx_res_t* c;
  frames_args_t a;
  const void* x;
  result_t r[3] = {{0}};   /* spectrum, times, frequencies */
  if (argc != 6 + f64 || !get_ctx(env, argv[0], &c) || !get_frames_args(env, argv + 2, f64, 0, &a) ||
      !get_rows(env, argv[1], c, mem, (size_t)(f64 ? 8 : 4) << cplx, a.batch, a.len, 1, &x))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  int rc = res_open(&r[0], c, mem, f64 ? 16 : 8, (uint64_t)a.batch, (uint64_t)a.out, (uint64_t)a.p.fft_length);
  if (!rc)
    rc = f64 ? (cplx ? nxsig_stft_c128(c->ctx, (const nxsig_c128*)x, a.len, a.batch, a.len, a.w.data, a.wf64, &a.p, (nxsig_c128*)r[0].data, NULL, mem)
                     : nxsig_stft_f64(c->ctx, (const double*)x, a.len, a.batch, a.len, a.w.data, a.wf64, &a.p, (nxsig_c128*)r[0].data, NULL, mem))
             : (cplx ? nxsig_stft_c64(c->ctx, (const nxsig_c64*)x, a.len, a.batch, a.len, (const float*)a.w.data, &a.p, (nxsig_c64*)r[0].data, NULL, mem)
                     : nxsig_stft_f32(c->ctx, (const float*)x, a.len, a.batch, a.len, (const float*)a.w.data, &a.p, (nxsig_c64*)r[0].data, NULL, mem));
  if (mem == NXSIG_DEVICE) return res_ok2(env, &r[0], rc, a.out);
  /* the times and frequencies binaries of a host result */
  if (!rc) rc = res_open(&r[1], NULL, NXSIG_HOST, 4, (uint64_t)a.out, 1, 1);
  if (!rc) rc = res_open(&r[2], NULL, NXSIG_HOST, 4, (uint64_t)a.p.fft_length, 1, 1);
  if (!rc) rc = nxsig_stft_times_f32(a.p.frame_length, a.p.sampling_rate, a.out, (float*)r[1].data);
  if (!rc) rc = nxsig_fft_frequencies_f32(a.p.sampling_rate, a.p.fft_length, 0, (float*)r[2].data);
  if (rc) return res_fail(env, r, 3, rc);
  return enif_make_tuple5(env, mk_atom(env, "ok"), res_term(env, &r[0]), enif_make_int64(env, a.out), res_term(env, &r[1]), res_term(env, &r[2]));
}
static ERL_NIF_TERM nif_stft(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return stft_any(env, argc, argv, 0, 0, NXSIG_HOST); }
static ERL_NIF_TERM nif_stft_c64(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return stft_any(env, argc, argv, 1, 0, NXSIG_HOST); }
static ERL_NIF_TERM nif_stft_f64(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return stft_any(env, argc, argv, 0, 1, NXSIG_HOST); }
static ERL_NIF_TERM nif_stft_c128(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return stft_any(env, argc, argv, 1, 1, NXSIG_HOST); }
static ERL_NIF_TERM nif_stft_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return stft_any(env, argc, argv, 0, 0, NXSIG_DEVICE); }
static ERL_NIF_TERM nif_stft_c64_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return stft_any(env, argc, argv, 1, 0, NXSIG_DEVICE); }

/* istft(ctx, z_bin, num_frames, batch, window_bin, params) -> {:ok, y_bin}
 * istft_c128(ctx, z_bin (c128), num_frames, batch, window_bin, window_is_f64, params) -> {:ok, y_bin (c128)}
 * istft_dev(ctx, z_buf, num_frames, batch, window_bin, params) -> {:ok, y_buf} */
static ERL_NIF_TERM istft_any(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[], int f64, int mem) {
  ctx_res_t* c;
  frames_args_t a;
  const void* z;
  result_t y = {0};
  const size_t elem = f64 ? 16 : 8;
  if (argc != 6 + f64 || !get_ctx(env, argv[0], &c) || !get_frames_args(env, argv + 2, f64, 1, &a) ||
      !get_rows(env, argv[1], c, mem, elem, a.batch, a.len, a.p.fft_length, &z))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  int rc = res_open(&y, c, mem, elem, (uint64_t)a.batch, (uint64_t)a.out, 1);
  if (!rc)
    rc = f64 ? nxsig_istft_c128(c->ctx, (const nxsig_c128*)z, a.len, a.batch, a.w.data, a.wf64, &a.p, (nxsig_c128*)y.data, mem)
             : nxsig_istft_c64(c->ctx, (const nxsig_c64*)z, a.len, a.batch, (const float*)a.w.data, &a.p, (nxsig_c64*)y.data, mem);
  return res_ok(env, &y, rc);
}
static ERL_NIF_TERM nif_istft(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return istft_any(env, argc, argv, 0, NXSIG_HOST); }
static ERL_NIF_TERM nif_istft_c128(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return istft_any(env, argc, argv, 1, NXSIG_HOST); }
static ERL_NIF_TERM nif_istft_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return istft_any(env, argc, argv, 0, NXSIG_DEVICE); }

/* istft_filtered(ctx, z_bin, num_frames, batch, window_bin, params, h_bin) -> {:ok, y_bin}
 * NxSignal.istft(Nx.multiply(z, hfft), window, opts) in one library call (guides/filtering.livemd:141 + :150-157)
 * istft_filtered_dev(ctx, z_buf, num_frames, batch, window_bin, params, h_bin) -> {:ok, y_buf}   (z_buf is left untouched) */
static ERL_NIF_TERM istft_filtered_any(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[], int mem) {
  ctx_res_t* c;
  frames_args_t a;
  ErlNifBinary h;
  const void* z;
  result_t y = {0};
  if (argc != 7 || !get_ctx(env, argv[0], &c) || !get_frames_args(env, argv + 2, 0, 1, &a) || !enif_inspect_binary(env, argv[6], &h) ||
      h.size != (size_t)a.p.fft_length * 8 || !get_rows(env, argv[1], c, mem, 8, a.batch, a.len, a.p.fft_length, &z))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  int rc = res_open(&y, c, mem, 8, (uint64_t)a.batch, (uint64_t)a.out, 1);
  if (!rc)
    rc = nxsig_istft_filtered_c64(c->ctx, (const nxsig_c64*)z, a.len, a.batch, (const float*)a.w.data, &a.p, (const nxsig_c64*)h.data,
                                  (nxsig_c64*)y.data, mem);
  return res_ok(env, &y, rc);
}
static ERL_NIF_TERM nif_istft_filtered(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return istft_filtered_any(env, argc, argv, NXSIG_HOST); }
static ERL_NIF_TERM nif_istft_filtered_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return istft_filtered_any(env, argc, argv, NXSIG_DEVICE); }

/* The argument run the FIR NIFs have at argv[2 ...]: length, batch, taps_bin (f32, or f64 on the f64 tier), mode; `out` as in
 * frames_args_t: nxsig_conv_length(length, taps, mode) samples per result row, or the library's status */
typedef struct {
  ErlNifSInt64 len;
  int batch, taps, mode;
  ErlNifBinary h;
  int64_t out;
} fir_args_t;
static int get_fir_args(ErlNifEnv* env, const ERL_NIF_TERM* argv, size_t elem, fir_args_t* a) {
  if (!enif_get_int64(env, argv[0], &a->len) || !enif_get_int(env, argv[1], &a->batch) || !enif_inspect_binary(env, argv[2], &a->h) ||
      !enif_get_int(env, argv[3], &a->mode))
    return 0;
  if (a->batch < 1 || a->len < 1 || a->h.size < elem || a->h.size % elem || a->h.size / elem > 0x7fffffff) return 0;
  a->taps = (int)(a->h.size / elem);
  a->out = nxsig_conv_length(a->len, a->taps, a->mode);
  return 1;
}

/* fir(ctx, x_bin, length, batch, taps_bin, mode) -> {:ok, y_bin}   (Convolution.convolve(method: :fft), real 1-D rows)
 * fir_f64(ctx, x_bin (f64), length, batch, taps_bin (f64), mode) -> {:ok, y_bin (f64)}
 * fir_dev(ctx, x_buf, length, batch, taps_bin, mode) -> {:ok, y_buf, out_length} */
static ERL_NIF_TERM fir_any(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[], int f64, int mem) {
  ctx_res_t* c;
  fir_args_t a;
  const void* x;
  result_t y = {0};
  const size_t elem = f64 ? 8 : 4;
  if (argc != 6 || !get_ctx(env, argv[0], &c) || !get_fir_args(env, argv + 2, elem, &a) ||
      !get_rows(env, argv[1], c, mem, elem, a.batch, a.len, 1, &x))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  int rc = res_open(&y, c, mem, elem, (uint64_t)a.batch, (uint64_t)a.out, 1);
  if (!rc)
    rc = f64 ? nxsig_fir_f64(c->ctx, (const double*)x, a.len, a.batch, a.len, (const double*)a.h.data, a.taps, a.mode, (double*)y.data, mem)
             : nxsig_fir_f32(c->ctx, (const float*)x, a.len, a.batch, a.len, (const float*)a.h.data, a.taps, a.mode, (float*)y.data, mem);
  return mem == NXSIG_DEVICE ? res_ok2(env, &y, rc, a.out) : res_ok(env, &y, rc);
}
static ERL_NIF_TERM nif_fir(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return fir_any(env, argc, argv, 0, NXSIG_HOST); }
static ERL_NIF_TERM nif_fir_f64(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return fir_any(env, argc, argv, 1, NXSIG_HOST); }
static ERL_NIF_TERM nif_fir_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return fir_any(env, argc, argv, 0, NXSIG_DEVICE); }

/* as_windowed(ctx, x_bin, length, batch, window_length, stride, pad_mode, pad_lo, pad_hi) -> {:ok, frames_bin, num_frames}
 * as_windowed_f64: the same on f64 binaries */
static ERL_NIF_TERM as_windowed_any(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[], int f64) {
  ctx_res_t* c;
  ErlNifSInt64 length, lo, hi;
  int batch, wl, stride, pad;
  const void* x;
  result_t o = {0};
  const size_t elem = f64 ? 8 : 4;
  if (argc != 9 || !get_ctx(env, argv[0], &c) || !enif_get_int64(env, argv[2], &length) || !enif_get_int(env, argv[3], &batch) ||
      !enif_get_int(env, argv[4], &wl) || !enif_get_int(env, argv[5], &stride) || !enif_get_int(env, argv[6], &pad) ||
      !enif_get_int64(env, argv[7], &lo) || !enif_get_int64(env, argv[8], &hi) ||
      !get_rows(env, argv[1], c, NXSIG_HOST, elem, batch, length, 1, &x))
    return enif_make_badarg(env);
  int64_t m = nxsig_num_frames(length, wl, stride, pad, lo, hi);
  if (m < 0) return mk_error(env, (int)m);
  int rc = res_open(&o, c, NXSIG_HOST, elem, (uint64_t)batch, (uint64_t)m, (uint64_t)wl);
  if (!rc)
    rc = f64 ? nxsig_as_windowed_f64(c->ctx, (const double*)x, length, batch, length, wl, stride, pad, lo, hi, (double*)o.data, NULL, NXSIG_HOST)
             : nxsig_as_windowed_f32(c->ctx, (const float*)x, length, batch, length, wl, stride, pad, lo, hi, (float*)o.data, NULL, NXSIG_HOST);
  return res_ok2(env, &o, rc, m);
}
static ERL_NIF_TERM nif_as_windowed(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return as_windowed_any(env, argc, argv, 0); }
static ERL_NIF_TERM nif_as_windowed_f64(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return as_windowed_any(env, argc, argv, 1); }

/* overlap_and_add(ctx, frames_bin, num_frames, batch, frame_length, overlap_length, components) -> {:ok, out_bin}
 * overlap_and_add_f64: the same on f64 (components 1) / c128 (2) binaries */
static ERL_NIF_TERM overlap_and_add_any(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[], int f64) {
  ctx_res_t* c;
  ErlNifSInt64 m;
  int batch, n, overlap, comps;
  const void* f;
  result_t o = {0};
  const size_t elem = f64 ? 8 : 4;
  if (argc != 7 || !get_ctx(env, argv[0], &c) || !enif_get_int64(env, argv[2], &m) || !enif_get_int(env, argv[3], &batch) ||
      !enif_get_int(env, argv[4], &n) || !enif_get_int(env, argv[5], &overlap) || !enif_get_int(env, argv[6], &comps) ||
      (comps != 1 && comps != 2) || !get_rows(env, argv[1], c, NXSIG_HOST, elem * (size_t)comps, batch, m, n, &f))
    return enif_make_badarg(env);
  /* the reference's own check (lib/nx_signal.ex:692-695) must surface as ArgumentError, not badarg: let the library say it */
  int64_t out_len = (overlap >= 0 && overlap < n) ? m * (int64_t)(n - overlap) + overlap : 1;
  int rc = res_open(&o, c, NXSIG_HOST, elem, (uint64_t)batch, (uint64_t)out_len, (uint64_t)comps);
  if (!rc)
    rc = f64 ? nxsig_overlap_and_add_f64(c->ctx, (const double*)f, m, batch, n, overlap, comps, (double*)o.data, NXSIG_HOST)
             : nxsig_overlap_and_add(c->ctx, (const float*)f, m, batch, n, overlap, comps, (float*)o.data, NXSIG_HOST);
  return res_ok(env, &o, rc);
}
static ERL_NIF_TERM nif_overlap_and_add(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return overlap_and_add_any(env, argc, argv, 0); }
static ERL_NIF_TERM nif_overlap_and_add_f64(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return overlap_and_add_any(env, argc, argv, 1); }

/* fft(ctx, in_bin, in_is_real, rows, n_in, fft_length, inverse) -> {:ok, c64 binary}   (Nx.fft / Nx.ifft over the last axis)
 * fft_c128: the same -> {:ok, c128 binary}   (Nx.fft / Nx.ifft of f64 / c128 rows) */
static ERL_NIF_TERM fft_any(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[], int f64) {
  ctx_res_t* c;
  ErlNifSInt64 rows;
  int is_real, n_in, k, inv;
  const void* in;
  result_t o = {0};
  const size_t real = f64 ? 8 : 4;
  if (argc != 7 || !get_ctx(env, argv[0], &c) || !enif_get_int(env, argv[2], &is_real) || !enif_get_int64(env, argv[3], &rows) ||
      !enif_get_int(env, argv[4], &n_in) || !enif_get_int(env, argv[5], &k) || !enif_get_int(env, argv[6], &inv) || k < 1 ||
      !get_rows(env, argv[1], c, NXSIG_HOST, is_real ? real : 2 * real, rows, n_in, 1, &in))
    return enif_make_badarg(env);
  int rc = res_open(&o, c, NXSIG_HOST, 2 * real, (uint64_t)rows, (uint64_t)k, 1);
  if (!rc)
    rc = f64 ? nxsig_fft_c128(c->ctx, in, is_real, rows, n_in, k, inv, (nxsig_c128*)o.data, NXSIG_HOST)
             : nxsig_fft(c->ctx, in, is_real, rows, n_in, k, inv, (nxsig_c64*)o.data, NXSIG_HOST);
  return res_ok(env, &o, rc);
}
static ERL_NIF_TERM nif_fft(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return fft_any(env, argc, argv, 0); }
static ERL_NIF_TERM nif_fft_c128(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return fft_any(env, argc, argv, 1); }

/* fftconvolve_c64(ctx, a_bin, b_bin, mode) -> {:ok, c64 binary}   (1-D complex case of Convolution.fftconvolve/3) */
static ERL_NIF_TERM nif_fftconvolve_c64(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  ErlNifBinary a, b;
  int mode;
  result_t o = {0};
  if (argc != 4 || !get_ctx(env, argv[0], &c) || !enif_inspect_binary(env, argv[1], &a) || !enif_inspect_binary(env, argv[2], &b) ||
      !enif_get_int(env, argv[3], &mode) || a.size < 8 || b.size < 8 || a.size % 8 || b.size % 8)
    return enif_make_badarg(env);
  int64_t n = nxsig_conv_length((int64_t)(a.size / 8), (int64_t)(b.size / 8), mode);
  if (n < 0) return mk_error(env, (int)n);
  int rc = res_open(&o, c, NXSIG_HOST, 8, (uint64_t)n, 1, 1);
  if (!rc)
    rc = nxsig_fftconvolve_c64(c->ctx, (const nxsig_c64*)a.data, (int64_t)(a.size / 8), (const nxsig_c64*)b.data, (int64_t)(b.size / 8), mode,
                               (nxsig_c64*)o.data, NXSIG_HOST);
  return res_ok(env, &o, rc);
}

static int get_i64_list(ErlNifEnv* env, ERL_NIF_TERM list, int64_t* out, unsigned cap, unsigned* n) {
  ERL_NIF_TERM head, tail = list;
  if (!enif_get_list_length(env, list, n) || *n > cap) return 0;
  for (unsigned i = 0; i < *n; ++i) {
    ErlNifSInt64 v;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_int64(env, head, &v)) return 0;
    out[i] = v;
  }
  return 1;
}
/* a shape list of rank 1 .. 8 without an empty dimension; *n = its element count */
static int get_shape(ErlNifEnv* env, ERL_NIF_TERM list, int64_t* shape, unsigned* rank, size_t* n) {
  if (!get_i64_list(env, list, shape, 8, rank) || *rank < 1) return 0;
  *n = 1;
  for (unsigned d = 0; d < *rank; ++d)
    if (shape[d] < 1 || !mul_size(n, (uint64_t)shape[d])) return 0;
  return 1;
}

/* fft_nd(ctx, in_bin, in_is_real, shape, axes, lengths, inverse) -> {:ok, c64 binary}   (Transforms.fft_nd / ifft_nd, any axes) */
static ERL_NIF_TERM nif_fft_nd(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  int is_real, inv;
  int64_t shape[8], axes64[16], lengths[16], osh[8];
  int32_t axes[16];
  unsigned rank, na, nl;
  size_t n_in, n_out = 1;
  const void* in;
  result_t o = {0};
  if (argc != 7 || !get_ctx(env, argv[0], &c) || !enif_get_int(env, argv[2], &is_real) || !get_shape(env, argv[3], shape, &rank, &n_in) ||
      !get_i64_list(env, argv[4], axes64, 16, &na) || !get_i64_list(env, argv[5], lengths, 16, &nl) || !enif_get_int(env, argv[6], &inv) ||
      na != nl || !get_rows(env, argv[1], c, NXSIG_HOST, is_real ? 4 : 8, (int64_t)n_in, 1, 1, &in))
    return enif_make_badarg(env);
  memcpy(osh, shape, sizeof osh);
  for (unsigned i = 0; i < na; ++i) {
    int64_t ax = axes64[i] < 0 ? axes64[i] + (int64_t)rank : axes64[i];
    if (ax < 0 || ax >= (int64_t)rank || lengths[i] < 1) return enif_make_badarg(env);
    axes[i] = (int32_t)ax; osh[ax] = lengths[i];
  }
  for (unsigned d = 0; d < rank; ++d) if (!mul_size(&n_out, (uint64_t)osh[d])) return mk_oom(env);
  int rc = res_open(&o, c, NXSIG_HOST, 8, n_out, 1, 1);
  if (!rc) rc = nxsig_fft_nd(c->ctx, in, is_real, shape, (int32_t)rank, axes, lengths, (int32_t)na, inv, (nxsig_c64*)o.data, NXSIG_HOST);
  return res_ok(env, &o, rc);
}

/* fftconvolve_nd(ctx, a_bin, a_is_real, a_shape, b_bin, b_is_real, b_shape, mode) -> {:ok, out_bin, out_shape}
 * (Convolution.fftconvolve/3 for operands of equal rank; out is f32 when both are real, else c64) */
typedef int (*conv_nd_fn)(nxsig_ctx*, const void*, int32_t, const int64_t*, const void*, int32_t, const int64_t*, int32_t, int32_t, void*,
                          int64_t*, int32_t);
static ERL_NIF_TERM conv_nd_common(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[], conv_nd_fn fn, const char* rank_msg) {
  ctx_res_t* c;
  ErlNifBinary a, b;
  int a_real, b_real, mode;
  int64_t s1[8], s2[8], osh[8];
  unsigned r1, r2;
  result_t o = {0};
  if (argc != 8 || !get_ctx(env, argv[0], &c) || !enif_inspect_binary(env, argv[1], &a) || !enif_get_int(env, argv[2], &a_real) ||
      !get_i64_list(env, argv[3], s1, 8, &r1) || !enif_inspect_binary(env, argv[4], &b) || !enif_get_int(env, argv[5], &b_real) ||
      !get_i64_list(env, argv[6], s2, 8, &r2) || !enif_get_int(env, argv[7], &mode) || r1 < 1)
    return enif_make_badarg(env);
  if (r1 != r2) return mk_error_msg(env, NXSIG_ERR_INVALID_ARG, rank_msg);
  size_t na = 1, nb = 1, nfull = 1;
  for (unsigned d = 0; d < r1; ++d) {
    if (s1[d] < 1 || s2[d] < 1 || !mul_size(&na, (uint64_t)s1[d]) || !mul_size(&nb, (uint64_t)s2[d]) ||
        !mul_size(&nfull, (uint64_t)(s1[d] + s2[d] - 1)))
      return enif_make_badarg(env);
  }
  if (a.size % (a_real ? 4 : 8) || a.size / (a_real ? 4 : 8) != na || b.size % (b_real ? 4 : 8) || b.size / (b_real ? 4 : 8) != nb)
    return enif_make_badarg(env);
  const size_t es = (a_real && b_real) ? 4 : 8;
  int rc = res_open(&o, c, NXSIG_HOST, es, nfull, 1, 1);  /* every mode's result fits the full size */
  if (!rc) rc = fn(c->ctx, a.data, a_real, s1, b.data, b_real, s2, (int32_t)r1, mode, o.data, osh, NXSIG_HOST);
  if (rc) return res_fail(env, &o, 1, rc);
  size_t nres = 1;
  ERL_NIF_TERM dims[8];
  for (unsigned d = 0; d < r1; ++d) { nres *= (size_t)osh[d]; dims[d] = enif_make_int64(env, osh[d]); }
  if (!enif_realloc_binary(&o.bin, nres * es)) return res_fail(env, &o, 1, RES_NOMEM);
  return mk_ok2(env, res_term(env, &o), enif_make_list_from_array(env, dims, r1));
}
static ERL_NIF_TERM nif_fftconvolve_nd(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  return conv_nd_common(env, argc, argv, nxsig_fftconvolve_nd, "Rank of in1 and in2 must be equal.");  /* convolution.ex:295-296 */
}
/* convolve_direct(ctx, a_bin, a_is_real, a_shape, b_bin, b_is_real, b_shape, mode) -> {:ok, out_bin, out_shape}
 * (Convolution.convolve/3 with its default method: time-domain sums, lib/nx_signal/convolution.ex:95-218) */
static ERL_NIF_TERM nif_convolve_direct(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  return conv_nd_common(env, argc, argv, nxsig_convolve_direct,
                        "NxSignal.convolve/3 requires both inputs to have the same rank or one of them to be a scalar");  /* :112-115 */
}

/* filter inputs: binary of prod(shape) f32 / f64 elements, shape and window lists of one length <= 8 */
static int filter_args(ErlNifEnv* env, const ERL_NIF_TERM argv[], ctx_res_t** c, const void** in, int* is_f64, int64_t* shape, int64_t* ks,
                       unsigned* rank, size_t* n) {
  unsigned r2;
  return get_ctx(env, argv[0], c) && enif_get_int(env, argv[2], is_f64) && get_shape(env, argv[3], shape, rank, n) &&
         get_i64_list(env, argv[4], ks, 8, &r2) && r2 == *rank && get_rows(env, argv[1], *c, NXSIG_HOST, *is_f64 ? 8 : 4, (int64_t)*n, 1, 1, in);
}

/* median(ctx, x_bin, is_f64, shape, kernel_shape) -> {:ok, f32 binary}   (Filters.median/2, lib/nx_signal/filters.ex:17-55) */
static ERL_NIF_TERM nif_median(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  const void* in;
  int is_f64;
  int64_t shape[8], ks[8];
  unsigned rank;
  size_t n;
  result_t o = {0};
  if (argc != 5 || !filter_args(env, argv, &c, &in, &is_f64, shape, ks, &rank, &n)) return enif_make_badarg(env);
  int rc = res_open(&o, c, NXSIG_HOST, 4, n, 1, 1);
  if (!rc) rc = nxsig_median_filter(c->ctx, in, is_f64, shape, (int32_t)rank, ks, (float*)o.data, NXSIG_HOST);
  return res_ok(env, &o, rc);
}

/* wiener(ctx, x_bin, is_f64, shape, kernel_size, has_noise, noise) -> {:ok, binary of x's type}   (Filters.wiener/2, filters.ex:81-110) */
static ERL_NIF_TERM nif_wiener(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  const void* in;
  int is_f64, has_noise;
  double noise;
  int64_t shape[8], ks[8];
  unsigned rank;
  size_t n;
  result_t o = {0};
  if (argc != 7 || !filter_args(env, argv, &c, &in, &is_f64, shape, ks, &rank, &n) || !enif_get_int(env, argv[5], &has_noise) ||
      !get_number(env, argv[6], &noise))
    return enif_make_badarg(env);
  int rc = res_open(&o, c, NXSIG_HOST, is_f64 ? 8 : 4, n, 1, 1);
  if (!rc) rc = nxsig_wiener(c->ctx, in, is_f64, shape, (int32_t)rank, ks, has_noise, noise, o.data, NULL, NXSIG_HOST);
  return res_ok(env, &o, rc);
}

/* resample_poly(ctx, x_bin, is_complex, length, batch, taps_bin, up, down) -> {:ok, y_bin, out_length}
 * (Filters.resample_poly/4: polyphase resampling of f32 / c64 rows by up / down, include/nxsig.h: nxsig_resample_poly; the taps are f32,
 * gain included)
 * resample_poly_dev(ctx, x_buf, is_complex, length, batch, taps_bin, up, down) -> {:ok, y_buf, out_length} */
static ERL_NIF_TERM resample_poly_any(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[], int mem) {
  ctx_res_t* c;
  ErlNifBinary h;
  ErlNifSInt64 length;
  int is_complex, batch, up, down;
  const void* x;
  result_t y = {0};
  if (argc != 8 || !get_ctx(env, argv[0], &c) || !enif_get_int(env, argv[2], &is_complex) || !enif_get_int64(env, argv[3], &length) ||
      !enif_get_int(env, argv[4], &batch) || !enif_inspect_binary(env, argv[5], &h) || !enif_get_int(env, argv[6], &up) ||
      !enif_get_int(env, argv[7], &down) || h.size % 4 || h.size / 4 > 0x7fffffff ||
      !get_rows(env, argv[1], c, mem, is_complex ? 8 : 4, batch, length, 1, &x))
    return enif_make_badarg(env);
  int64_t n = nxsig_resample_length(length, up, down);
  if (n < 0) return mk_error(env, (int)n);
  int rc = res_open(&y, c, mem, is_complex ? 8 : 4, (uint64_t)batch, (uint64_t)n, 1);
  if (!rc) rc = nxsig_resample_poly(c->ctx, x, is_complex, length, batch, length, (const float*)h.data, (int)(h.size / 4), up, down, y.data, mem);
  return res_ok2(env, &y, rc, n);
}
static ERL_NIF_TERM nif_resample_poly(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return resample_poly_any(env, argc, argv, NXSIG_HOST); }
static ERL_NIF_TERM nif_resample_poly_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return resample_poly_any(env, argc, argv, NXSIG_DEVICE); }

/* the arguments the welch and csd NIFs share, from argv[at]: length, batch, window_bin (f32), hop, fft_length, detrend, scaling, sampling_rate */
static int welch_args(ErlNifEnv* env, const ERL_NIF_TERM* argv, ErlNifSInt64* length, int* batch, ErlNifBinary* w, int* hop, int* fft_length,
                      int* detrend, int* scaling, double* fs) {
  return enif_get_int64(env, argv[0], length) && enif_get_int(env, argv[1], batch) && enif_inspect_binary(env, argv[2], w) &&
         enif_get_int(env, argv[3], hop) && enif_get_int(env, argv[4], fft_length) && enif_get_int(env, argv[5], detrend) &&
         enif_get_int(env, argv[6], scaling) && enif_get_double(env, argv[7], fs) && *batch >= 1 && *length >= 1 && w->size >= 4 &&
         w->size % 4 == 0 && w->size / 4 <= 0x7fffffff;
}

/* welch(ctx, x_bin, length, batch, window_bin, hop, fft_length, detrend, scaling, sampling_rate) -> {:ok, pxx_bin, bins}
   (Spectral.welch/3: Welch's averaged periodogram of real f32 rows, include/nxsig.h: nxsig_welch_f32) */
static ERL_NIF_TERM nif_welch(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  ErlNifBinary w;
  ErlNifSInt64 length;
  int batch, hop, fft_length, detrend, scaling;
  double fs;
  const void* x;
  result_t o = {0};
  if (argc != 10 || !get_ctx(env, argv[0], &c) || !welch_args(env, argv + 2, &length, &batch, &w, &hop, &fft_length, &detrend, &scaling, &fs) ||
      !get_rows(env, argv[1], c, NXSIG_HOST, 4, batch, length, 1, &x))
    return enif_make_badarg(env);
  int32_t nb = nxsig_welch_bins(fft_length);
  if (nb < 0) return mk_error(env, nb);
  int rc = res_open(&o, c, NXSIG_HOST, 4, (uint64_t)batch, (uint64_t)nb, 1);
  if (!rc)
    rc = nxsig_welch_f32(c->ctx, (const float*)x, length, batch, length, (const float*)w.data, (int)(w.size / 4), hop, fft_length, detrend, scaling,
                         fs, (float*)o.data, NXSIG_HOST);
  return res_ok2(env, &o, rc, nb);
}

/* csd(ctx, x_bin, y_bin, length, batch, window_bin, hop, fft_length, detrend, scaling, sampling_rate) -> {:ok, pxy_bin, pxx_bin, pyy_bin, bins}
   (Spectral.csd/4 and coherence/4: the cross spectrum c64 and both auto-spectra f32 of one call, nxsig_csd_f32) */
static ERL_NIF_TERM nif_csd(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  ErlNifBinary w;
  ErlNifSInt64 length;
  int batch, hop, fft_length, detrend, scaling;
  double fs;
  const void *x, *y;
  result_t r[3] = {{0}};   /* pxy, pxx, pyy */
  if (argc != 11 || !get_ctx(env, argv[0], &c) || !welch_args(env, argv + 3, &length, &batch, &w, &hop, &fft_length, &detrend, &scaling, &fs) ||
      !get_rows(env, argv[1], c, NXSIG_HOST, 4, batch, length, 1, &x) || !get_rows(env, argv[2], c, NXSIG_HOST, 4, batch, length, 1, &y))
    return enif_make_badarg(env);
  int32_t nb = nxsig_welch_bins(fft_length);
  if (nb < 0) return mk_error(env, nb);
  int rc = res_open(&r[0], c, NXSIG_HOST, 8, (uint64_t)batch, (uint64_t)nb, 1);
  if (!rc) rc = res_open(&r[1], c, NXSIG_HOST, 4, (uint64_t)batch, (uint64_t)nb, 1);
  if (!rc) rc = res_open(&r[2], c, NXSIG_HOST, 4, (uint64_t)batch, (uint64_t)nb, 1);
  if (!rc)
    rc = nxsig_csd_f32(c->ctx, (const float*)x, (const float*)y, length, batch, length, (const float*)w.data, (int)(w.size / 4), hop, fft_length,
                       detrend, scaling, fs, (float*)r[1].data, (float*)r[2].data, (nxsig_c64*)r[0].data, NXSIG_HOST);
  if (rc) return res_fail(env, r, 3, rc);
  return enif_make_tuple5(env, mk_atom(env, "ok"), res_term(env, &r[0]), res_term(env, &r[1]), res_term(env, &r[2]), enif_make_int(env, nb));
}

/* peak-finding shapes: rank 1 .. 8, no empty dimension, fewer than 2^32 elements (the library checks the rest) */
static int peaks_shape(ErlNifEnv* env, ERL_NIF_TERM list, int64_t* shape, unsigned* rank, size_t* n) {
  return get_shape(env, list, shape, rank, n) && *n < ((size_t)1 << 32);
}

/* argrelextrema(ctx, x_bin, dtype, shape, axis, shifts, comparator) -> {:ok, s32 [size][rank] binary, valid}
   (PeakFinding.argrelextrema/3, lib/nx_signal/peak_finding.ex; dtype nxsig_dtype, comparator nxsig_comparator) */
static ERL_NIF_TERM nif_argrelextrema(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  int dtype, axis, comparator;
  int64_t shape[8], shifts;
  unsigned rank;
  size_t n;
  const void* in;
  result_t o = {0};
  uint32_t valid = 0;
  if (argc != 7 || !get_ctx(env, argv[0], &c) || !enif_get_int(env, argv[2], &dtype) || !peaks_shape(env, argv[3], shape, &rank, &n) ||
      !enif_get_int(env, argv[4], &axis) || !enif_get_int64(env, argv[5], &shifts) || !enif_get_int(env, argv[6], &comparator) || dtype < 0 ||
      dtype > 5 || !get_rows(env, argv[1], c, NXSIG_HOST, dtype == 1 || dtype == 3 || dtype == 5 ? 8 : 4, (int64_t)n, 1, 1, &in))
    return enif_make_badarg(env);
  int rc = res_open(&o, c, NXSIG_HOST, 4, n, rank, 1);
  if (!rc) rc = nxsig_argrelextrema(c->ctx, in, dtype, shape, (int32_t)rank, axis, shifts, comparator, (int32_t*)o.data, &valid, NXSIG_HOST);
  return res_ok2(env, &o, rc, (int64_t)valid);
}

/* nonzero(ctx, mask_bin, shape) -> {:ok, s32 [size][rank] binary, valid}   (the compaction of argrelextrema/3 for a custom comparator's
   u8 mask) */
static ERL_NIF_TERM nif_nonzero(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  int64_t shape[8];
  unsigned rank;
  size_t n;
  const void* in;
  result_t o = {0};
  uint32_t valid = 0;
  if (argc != 3 || !get_ctx(env, argv[0], &c) || !peaks_shape(env, argv[2], shape, &rank, &n) ||
      !get_rows(env, argv[1], c, NXSIG_HOST, 1, (int64_t)n, 1, 1, &in))
    return enif_make_badarg(env);
  int rc = res_open(&o, c, NXSIG_HOST, 4, n, rank, 1);
  if (!rc) rc = nxsig_nonzero(c->ctx, (const uint8_t*)in, shape, (int32_t)rank, (int32_t*)o.data, &valid, NXSIG_HOST);
  return res_ok2(env, &o, rc, (int64_t)valid);
}

/* NxSignal.Waveforms (lib/nx_signal/waveforms.ex): t_bin holds f32 elements, or f64 when is_f64; results are binaries of t's type */
static int wave_args(ErlNifEnv* env, const ERL_NIF_TERM argv[], ctx_res_t** c, ErlNifBinary* in, int* is_f64, size_t* n) {
  if (!get_ctx(env, argv[0], c) || !enif_inspect_binary(env, argv[1], in) || !enif_get_int(env, argv[2], is_f64)) return 0;
  const size_t es = *is_f64 ? 8 : 4;
  *n = in->size / es;
  return in->size % es == 0;
}

/* sawtooth(ctx, t_bin, is_f64, width) -> {:ok, binary}   (Waveforms.sawtooth/2, waveforms.ex:29-54) */
static ERL_NIF_TERM nif_sawtooth(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  ErlNifBinary in;
  int is_f64;
  size_t n;
  double width;
  result_t o = {0};
  if (argc != 4 || !wave_args(env, argv, &c, &in, &is_f64, &n) || !get_number(env, argv[3], &width)) return enif_make_badarg(env);
  int rc = res_open(&o, c, NXSIG_HOST, is_f64 ? 8 : 4, n, 1, 1);
  if (!rc) rc = nxsig_sawtooth(c->ctx, in.data, is_f64, (int64_t)n, width, o.data, NXSIG_HOST);
  return res_ok(env, &o, rc);
}

/* square(ctx, t_bin, is_f64, duty, duty_bin) -> {:ok, s32 binary}   (Waveforms.square/2, waveforms.ex:96-104; a duty_bin of t's size
   replaces the number, an empty one means the number) */
static ERL_NIF_TERM nif_square(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  ErlNifBinary in, duty;
  int is_f64;
  size_t n;
  double d;
  result_t o = {0};
  if (argc != 5 || !wave_args(env, argv, &c, &in, &is_f64, &n) || !get_number(env, argv[3], &d) || !enif_inspect_binary(env, argv[4], &duty) ||
      (duty.size != 0 && duty.size != in.size))
    return enif_make_badarg(env);
  int rc = res_open(&o, c, NXSIG_HOST, 4, n, 1, 1);
  if (!rc) rc = nxsig_square(c->ctx, in.data, is_f64, (int64_t)n, d, duty.size ? duty.data : NULL, (int32_t*)o.data, NXSIG_HOST);
  return res_ok(env, &o, rc);
}

/* gaussian_pulse(ctx, t_bin, is_f64, center_frequency, bandwidth, bandwidth_reference_level) -> {:ok, envelope, in_phase, quadrature}
   (Waveforms.gaussian_pulse/2, waveforms.ex:161-198) */
static ERL_NIF_TERM nif_gaussian_pulse(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  ErlNifBinary in;
  int is_f64;
  size_t n;
  double fc, bw, bwr;
  result_t r[3] = {{0}};   /* envelope, in_phase, quadrature */
  if (argc != 6 || !wave_args(env, argv, &c, &in, &is_f64, &n) || !get_number(env, argv[3], &fc) || !get_number(env, argv[4], &bw) ||
      !get_number(env, argv[5], &bwr))
    return enif_make_badarg(env);
  int rc = 0;
  for (int i = 0; i < 3 && !rc; ++i) rc = res_open(&r[i], c, NXSIG_HOST, is_f64 ? 8 : 4, n, 1, 1);
  if (!rc) rc = nxsig_gaussian_pulse(c->ctx, in.data, is_f64, (int64_t)n, fc, bw, bwr, r[0].data, r[1].data, r[2].data, NXSIG_HOST);
  if (rc) return res_fail(env, r, 3, rc);
  return enif_make_tuple4(env, mk_atom(env, "ok"), res_term(env, &r[0]), res_term(env, &r[1]), res_term(env, &r[2]));
}

/* chirp(ctx, t_bin, is_f64, {f0, t1, f1}, method, vertex_zero, phi) -> {:ok, binary}   (Waveforms.chirp/5, waveforms.ex:249-300;
   method nxsig_chirp_method) */
static ERL_NIF_TERM nif_chirp(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  ErlNifBinary in;
  int is_f64, method, vertex_zero, arity;
  size_t n;
  const ERL_NIF_TERM* e;
  double f0, t1, f1, phi;
  result_t o = {0};
  if (argc != 7 || !wave_args(env, argv, &c, &in, &is_f64, &n) || !enif_get_tuple(env, argv[3], &arity, &e) || arity != 3 ||
      !get_number(env, e[0], &f0) || !get_number(env, e[1], &t1) || !get_number(env, e[2], &f1) || !enif_get_int(env, argv[4], &method) ||
      !enif_get_int(env, argv[5], &vertex_zero) || !get_number(env, argv[6], &phi))
    return enif_make_badarg(env);
  int rc = res_open(&o, c, NXSIG_HOST, is_f64 ? 8 : 4, n, 1, 1);
  if (!rc) rc = nxsig_chirp(c->ctx, in.data, is_f64, (int64_t)n, f0, t1, f1, method, vertex_zero, phi, o.data, NXSIG_HOST);
  return res_ok(env, &o, rc);
}

/* polynomial_sweep(ctx, t_bin, is_f64, coefs_f64_bin, phi, phi_degrees) -> {:ok, binary}   (Waveforms.polynomial_sweep/3,
   waveforms.ex:343-361) */
static ERL_NIF_TERM nif_polynomial_sweep(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  ErlNifBinary in, cf;
  int is_f64, degrees;
  size_t n;
  double phi, coefs[NXSIG_SWEEP_MAX_COEFS];
  result_t o = {0};
  if (argc != 6 || !wave_args(env, argv, &c, &in, &is_f64, &n) || !enif_inspect_binary(env, argv[3], &cf) || cf.size % 8 != 0 ||
      !get_number(env, argv[4], &phi) || !enif_get_int(env, argv[5], &degrees))
    return enif_make_badarg(env);
  const size_t nc = cf.size / 8;
  if (nc <= NXSIG_SWEEP_MAX_COEFS) memcpy(coefs, cf.data, cf.size);   /* a sub-binary need not be 8-byte aligned */
  int rc = res_open(&o, c, NXSIG_HOST, is_f64 ? 8 : 4, n, 1, 1);
  if (!rc)
    rc = nxsig_polynomial_sweep(c->ctx, in.data, is_f64, (int64_t)n, coefs, nc > NXSIG_SWEEP_MAX_COEFS ? -1 : (int32_t)nc, phi, degrees, o.data,
                                NXSIG_HOST);
  return res_ok(env, &o, rc);
}

/* unit_impulse(ctx, dtype, shape, index) -> {:ok, binary}   (Waveforms.unit_impulse/2, waveforms.ex:406-437; dtype nxsig_dtype, index
   one entry per axis) */
static ERL_NIF_TERM nif_unit_impulse(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  int dtype;
  int64_t shape[8], index[8];
  unsigned rank, r2;
  size_t n = 1;
  result_t o = {0};
  if (argc != 4 || !get_ctx(env, argv[0], &c) || !enif_get_int(env, argv[1], &dtype) || dtype < 0 || dtype > 5 ||
      !get_i64_list(env, argv[2], shape, 8, &rank) || !get_i64_list(env, argv[3], index, 8, &r2) || r2 != rank)
    return enif_make_badarg(env);
  for (unsigned d = 0; d < rank; ++d)
    if (shape[d] < 0 || !mul_size(&n, (uint64_t)shape[d])) return enif_make_badarg(env);
  int rc = res_open(&o, c, NXSIG_HOST, dtype == 1 || dtype == 3 || dtype == 5 ? 8 : 4, n, 1, 1);
  if (!rc) rc = nxsig_unit_impulse(c->ctx, dtype, shape, (int32_t)rank, index, o.data, NXSIG_HOST);
  return res_ok(env, &o, rc);
}

/* stft_to_mel(ctx, z_bin, rows, fft_length, mel_bins, filters_bin) -> {:ok, f32[rows][mel_bins]}   (lib/nx_signal.ex:486-513) */
static ERL_NIF_TERM nif_stft_to_mel(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  ErlNifSInt64 rows;
  int k, bins;
  const void *z, *f;
  result_t o = {0};
  if (argc != 6 || !get_ctx(env, argv[0], &c) || !enif_get_int64(env, argv[2], &rows) || !enif_get_int(env, argv[3], &k) ||
      !enif_get_int(env, argv[4], &bins) || !get_rows(env, argv[1], c, NXSIG_HOST, 8, rows, k, 1, &z) ||
      !get_rows(env, argv[5], c, NXSIG_HOST, 4, bins, k, 1, &f))
    return enif_make_badarg(env);
  int rc = res_open(&o, c, NXSIG_HOST, 4, (uint64_t)rows, (uint64_t)bins, 1);
  if (!rc) rc = nxsig_stft_to_mel(c->ctx, (const nxsig_c64*)z, rows, k, bins, (const float*)f, (float*)o.data, NXSIG_HOST);
  return res_ok(env, &o, rc);
}

/* stft_mel(ctx, x_bin, length, batch, window_bin, params, mel_bins, filters_bin) -> {:ok, f32[batch][M][mel_bins], M}  (fused) */
static ERL_NIF_TERM nif_stft_mel(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  frames_args_t a;
  int bins;
  const void *x, *f;
  result_t o = {0};
  if (argc != 8 || !get_ctx(env, argv[0], &c) || !get_frames_args(env, argv + 2, 0, 0, &a) || !enif_get_int(env, argv[6], &bins) ||
      !get_rows(env, argv[1], c, NXSIG_HOST, 4, a.batch, a.len, 1, &x) || !get_rows(env, argv[7], c, NXSIG_HOST, 4, bins, a.p.fft_length, 1, &f))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  int rc = res_open(&o, c, NXSIG_HOST, 4, (uint64_t)a.batch, (uint64_t)a.out, (uint64_t)bins);
  if (!rc)
    rc = nxsig_stft_mel_f32(c->ctx, (const float*)x, a.len, a.batch, a.len, (const float*)a.w.data, &a.p, bins, (const float*)f, (float*)o.data,
                            NULL, NXSIG_HOST);
  return res_ok2(env, &o, rc, a.out);
}

/* stft_magnitude(ctx, x_bin, length, batch, window_bin, params, kind) -> {:ok, f32[batch][M][fft_length / 2], M}
 * (fused |s| / |s|^2 / dBFS spectrogram of guides/spectrogram.livemd:76-92; kind 0 abs, 1 power, 2 dbfs) */
static ERL_NIF_TERM nif_stft_magnitude(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  frames_args_t a;
  int kind;
  const void* x;
  result_t o = {0};
  if (argc != 7 || !get_ctx(env, argv[0], &c) || !get_frames_args(env, argv + 2, 0, 0, &a) || !enif_get_int(env, argv[6], &kind) ||
      a.p.fft_length < 2 || !get_rows(env, argv[1], c, NXSIG_HOST, 4, a.batch, a.len, 1, &x))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  int rc = res_open(&o, c, NXSIG_HOST, 4, (uint64_t)a.batch, (uint64_t)a.out, (uint64_t)(a.p.fft_length / 2));
  if (!rc)
    rc = nxsig_stft_magnitude_f32(c->ctx, (const float*)x, a.len, a.batch, a.len, (const float*)a.w.data, &a.p, kind, (float*)o.data, NULL,
                                  NXSIG_HOST);
  return res_ok2(env, &o, rc, a.out);
}

/* ------------------------------------------------------------------------------------------------ device-resident tensors */
static ERL_NIF_TERM nif_to_device(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  ErlNifBinary b;
  result_t d = {0};
  if (argc != 2 || !get_ctx(env, argv[0], &c) || !enif_inspect_binary(env, argv[1], &b)) return enif_make_badarg(env);
  int rc = res_open(&d, c, NXSIG_DEVICE, 1, b.size, 1, 1);
  if (!rc) rc = nxsig_upload(c->ctx, d.data, b.data, b.size);
  return res_ok(env, &d, rc);
}

static ERL_NIF_TERM nif_from_device(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  buf_res_t* b;
  ErlNifBinary ob;
  if (argc != 1 || !get_buf(env, argv[0], &b)) return enif_make_badarg(env);
  nxsig_ctx* bc = buf_ctx(b);
  if (!bc) return enif_make_badarg(env);
  if (!enif_alloc_binary(b->bytes, &ob)) return mk_oom(env);
  int rc = nxsig_download(bc, ob.data, b->dptr, b->bytes);
  if (rc) { enif_release_binary(&ob); return mk_error(env, rc); }
  return mk_ok(env, enif_make_binary(env, &ob));
}

static ERL_NIF_TERM nif_buf_size(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  buf_res_t* b;
  if (argc != 1 || !get_buf(env, argv[0], &b)) return enif_make_badarg(env);
  return enif_make_int64(env, (ErlNifSInt64)b->bytes);
}

/* stft_onesided_dev / stft_packed_dev(ctx, x_buf, length, batch, window_bin, params) -> {:ok, z_buf, num_frames}
 * c64[batch][M][fft_length / 2]: bins 0 .. fft_length/2 - 1; packed: the imaginary part of bin 0 carries Re X[fft_length / 2] */
static ERL_NIF_TERM stft_half_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[], int packed) {
  ctx_res_t* c;
  frames_args_t a;
  const void* x;
  result_t z = {0};
  if (argc != 6 || !get_ctx(env, argv[0], &c) || !get_frames_args(env, argv + 2, 0, 0, &a) || a.p.fft_length < 2 ||
      !get_rows(env, argv[1], c, NXSIG_DEVICE, 4, a.batch, a.len, 1, &x))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  int rc = res_open(&z, c, NXSIG_DEVICE, 8, (uint64_t)a.batch, (uint64_t)a.out, (uint64_t)(a.p.fft_length / 2));
  if (!rc)
    rc = packed ? nxsig_stft_packed_f32(c->ctx, (const float*)x, a.len, a.batch, a.len, (const float*)a.w.data, &a.p, (nxsig_c64*)z.data, NULL, NXSIG_DEVICE)
                : nxsig_stft_onesided_f32(c->ctx, (const float*)x, a.len, a.batch, a.len, (const float*)a.w.data, &a.p, (nxsig_c64*)z.data, NULL, NXSIG_DEVICE);
  return res_ok2(env, &z, rc, a.out);
}
static ERL_NIF_TERM nif_stft_onesided_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return stft_half_dev(env, argc, argv, 0); }
static ERL_NIF_TERM nif_stft_packed_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) { return stft_half_dev(env, argc, argv, 1); }

/* istft_packed_dev(ctx, z_buf, num_frames, batch, window_bin, params) -> {:ok, y_buf}: z packed c64[batch][M][fft_length / 2],
 * y REAL f32[batch][M * hop + frame_length - hop] */
static ERL_NIF_TERM nif_istft_packed_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  frames_args_t a;
  const void* z;
  result_t y = {0};
  if (argc != 6 || !get_ctx(env, argv[0], &c) || !get_frames_args(env, argv + 2, 0, 1, &a) || a.p.fft_length < 2 ||
      !get_rows(env, argv[1], c, NXSIG_DEVICE, 8, a.batch, a.len, a.p.fft_length / 2, &z))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  int rc = res_open(&y, c, NXSIG_DEVICE, 4, (uint64_t)a.batch, (uint64_t)a.out, 1);
  if (!rc) rc = nxsig_istft_packed_f32(c->ctx, (const nxsig_c64*)z, a.len, a.batch, (const float*)a.w.data, &a.p, (float*)y.data, NXSIG_DEVICE);
  return res_ok(env, &y, rc);
}

/* spectrum_mul_dev(ctx, z_buf, rows, fft_length, h_bin) -> {:ok, z_buf}   (in place: Nx.multiply(z, hfft), guides/filtering.livemd:141) */
static ERL_NIF_TERM nif_spectrum_mul_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  ErlNifBinary h;
  ErlNifSInt64 rows;
  int k;
  const void* z;
  if (argc != 5 || !get_ctx(env, argv[0], &c) || !enif_get_int64(env, argv[2], &rows) || !enif_get_int(env, argv[3], &k) ||
      !enif_inspect_binary(env, argv[4], &h) || !get_rows(env, argv[1], c, NXSIG_DEVICE, 8, rows, k, 1, &z) || h.size != (size_t)k * 8)
    return enif_make_badarg(env);
  int rc = nxsig_spectrum_mul_c64(c->ctx, (const nxsig_c64*)z, rows, k, (const nxsig_c64*)h.data, (nxsig_c64*)z, NXSIG_DEVICE);
  return rc ? mk_error(env, rc) : mk_ok(env, argv[1]);
}

/* ---- time-frequency masks (nxsig_spectrum_mask_c64 / nxsig_istft_masked_c64).  z and mask are BOTH binaries (host result: a binary)
 * or BOTH device buffers of this context (result: a new buffer; the call is asynchronous).  mask_kind: 0 real f32[K], 1 one-sided
 * real f32[K/2 + 1], 2 c64[K] per frame; z_rows / mask_rows are equal or one of them is 1 (that operand is broadcast).
 * Reads both operands (binaries: exactly the size the counts give; buffers: at least); *mem = where they live, *rows = rows of the result */
static int get_masked(ErlNifEnv* env, ctx_res_t* c, ERL_NIF_TERM zt, int z_rows, ERL_NIF_TERM mt, int mask_kind, int mask_rows, int64_t m, int k,
                      const void** z, const void** mask, int* mem, int* rows) {
  if (mask_kind < 0 || mask_kind > 2 || (mask_kind == 1 && (k & 1))) return 0;
  if (z_rows != mask_rows && z_rows != 1 && mask_rows != 1) return 0;
  *mem = term_mem(env, zt);
  *rows = z_rows > mask_rows ? z_rows : mask_rows;
  return get_rows(env, zt, c, *mem, 8, z_rows, m, k, z) &&
         get_rows(env, mt, c, *mem, mask_kind == 2 ? 8 : 4, mask_rows, m, mask_kind == 1 ? k / 2 + 1 : k, mask);
}

/* spectrum_mask(ctx, z, z_rows, mask, mask_kind, mask_rows, num_frames, fft_length) -> {:ok, out}   (Nx.multiply(z, mask)) */
static ERL_NIF_TERM nif_spectrum_mask(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  ErlNifSInt64 m;
  int z_rows, kind, mask_rows, k, rows, mem;
  const void *z, *mask;
  result_t o = {0};
  if (argc != 8 || !get_ctx(env, argv[0], &c) || !enif_get_int(env, argv[2], &z_rows) || !enif_get_int(env, argv[4], &kind) ||
      !enif_get_int(env, argv[5], &mask_rows) || !enif_get_int64(env, argv[6], &m) || !enif_get_int(env, argv[7], &k) ||
      !get_masked(env, c, argv[1], z_rows, argv[3], kind, mask_rows, m, k, &z, &mask, &mem, &rows))
    return enif_make_badarg(env);
  int rc = res_open(&o, c, mem, 8, (uint64_t)rows, (uint64_t)m, (uint64_t)k);
  if (!rc) rc = nxsig_spectrum_mask_c64(c->ctx, (const nxsig_c64*)z, z_rows, mask, kind, mask_rows, m, k, (nxsig_c64*)o.data, mem);
  return res_ok(env, &o, rc);
}

/* istft_masked(ctx, z, z_rows, num_frames, window_bin, params, mask, mask_kind, mask_rows) -> {:ok, y}
 * NxSignal.istft(Nx.multiply(z, mask), window, opts) in one library call; z and mask are left untouched */
static ERL_NIF_TERM nif_istft_masked(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  ctx_res_t* c;
  ErlNifBinary w;
  ErlNifSInt64 m;
  int z_rows, kind, mask_rows, rows, mem;
  nxsig_stft_params p;
  const void *z, *mask;
  result_t y = {0};
  if (argc != 9 || !get_ctx(env, argv[0], &c) || !enif_get_int(env, argv[2], &z_rows) || !enif_get_int64(env, argv[3], &m) ||
      !enif_inspect_binary(env, argv[4], &w) || !get_params(env, argv[5], &p) || !enif_get_int(env, argv[7], &kind) ||
      !enif_get_int(env, argv[8], &mask_rows) || w.size != (size_t)p.frame_length * 4 ||
      !get_masked(env, c, argv[1], z_rows, argv[6], kind, mask_rows, m, p.fft_length, &z, &mask, &mem, &rows))
    return enif_make_badarg(env);
  int64_t n = nxsig_ola_length(m, p.frame_length, p.hop);
  if (n < 0) return mk_error(env, (int)n);
  int rc = res_open(&y, c, mem, 8, (uint64_t)rows, (uint64_t)n, 1);
  if (!rc)
    rc = nxsig_istft_masked_c64(c->ctx, (const nxsig_c64*)z, z_rows, m, (const float*)w.data, &p, mask, kind, mask_rows, (nxsig_c64*)y.data, mem);
  return res_ok(env, &y, rc);
}

/* ------------------------------------------------------------------------------------------------ multi-GPU groups
 * One BEAM process drives every GPU of the node: a LOCAL group (ncclCommInitAll).  The vectorized (multichannel) axis of the
 * reference (lib/nx_signal.ex:358-363) is what `axis = 0` shards. */
#define NXSIG_MAX_MEMBERS 64

/* group_create([device_id]) -> {:ok, group} */
static ERL_NIF_TERM nif_group_create(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  unsigned len;
  int32_t devs[NXSIG_MAX_MEMBERS];
  if (argc != 1 || !enif_get_list_length(env, argv[0], &len) || len < 1 || len > NXSIG_MAX_MEMBERS) return enif_make_badarg(env);
  ERL_NIF_TERM head, tail = argv[0];
  for (unsigned i = 0; i < len; ++i) {
    int d;
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_int(env, head, &d)) return enif_make_badarg(env);
    devs[i] = d;
  }
  nxsig_group* g = NULL;
  int rc = nxsig_group_create_local((int32_t)len, devs, &g);
  if (rc) return mk_error(env, rc);
  grp_res_t* r = enif_alloc_resource(GRP_RES, sizeof *r);
  r->grp = g;
  ERL_NIF_TERM t = enif_make_resource(env, r);
  enif_release_resource(r);
  return mk_ok(env, t);
}

/* group_info(group) -> {world, local_count, has_rccl} */
static ERL_NIF_TERM nif_group_info(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  grp_res_t* g;
  if (argc != 1 || !get_grp(env, argv[0], &g)) return enif_make_badarg(env);
  return enif_make_tuple3(env, enif_make_int(env, nxsig_group_world(g->grp)), enif_make_int(env, nxsig_group_local_count(g->grp)),
                          enif_make_int(env, nxsig_group_has_rccl(g->grp)));
}

/* The sharded calls over HOST tensors: the whole tensor goes in as element 0 of the per-member pointer array, the whole result comes
 * back the same way (include/nxsig.h, mem == NXSIG_HOST); the library splits and assembles. */
/* stft_sharded(group, x_bin, length, batch, window_bin, params, axis, gather) -> {:ok, z_bin, num_frames} */
static ERL_NIF_TERM nif_stft_sharded(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  grp_res_t* g;
  frames_args_t a;
  int axis, gather;
  const void* x;
  result_t z = {0};
  if (argc != 8 || !get_grp(env, argv[0], &g) || !get_frames_args(env, argv + 2, 0, 0, &a) || !enif_get_int(env, argv[6], &axis) ||
      !enif_get_int(env, argv[7], &gather) || !get_rows(env, argv[1], NULL, NXSIG_HOST, 4, a.batch, a.len, 1, &x))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  int rc = res_open(&z, NULL, NXSIG_HOST, 8, (uint64_t)a.batch, (uint64_t)a.out, (uint64_t)a.p.fft_length);
  const float* xs[NXSIG_MAX_MEMBERS] = {(const float*)x};
  nxsig_c64* zs[NXSIG_MAX_MEMBERS] = {(nxsig_c64*)z.data};
  if (!rc) rc = nxsig_stft_sharded_f32(g->grp, xs, a.len, a.batch, a.len, (const float*)a.w.data, &a.p, axis, gather, zs, NXSIG_HOST);
  return res_ok2(env, &z, rc, a.out);
}

/* istft_sharded(group, z_bin, num_frames, batch, window_bin, params, axis, gather) -> {:ok, y_bin} */
static ERL_NIF_TERM nif_istft_sharded(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  grp_res_t* g;
  frames_args_t a;
  int axis, gather;
  const void* z;
  result_t y = {0};
  if (argc != 8 || !get_grp(env, argv[0], &g) || !get_frames_args(env, argv + 2, 0, 1, &a) || !enif_get_int(env, argv[6], &axis) ||
      !enif_get_int(env, argv[7], &gather) || !get_rows(env, argv[1], NULL, NXSIG_HOST, 8, a.batch, a.len, a.p.fft_length, &z))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  int rc = res_open(&y, NULL, NXSIG_HOST, 8, (uint64_t)a.batch, (uint64_t)a.out, 1);
  const nxsig_c64* zs[NXSIG_MAX_MEMBERS] = {(const nxsig_c64*)z};
  nxsig_c64* ys[NXSIG_MAX_MEMBERS] = {(nxsig_c64*)y.data};
  if (!rc) rc = nxsig_istft_sharded_c64(g->grp, zs, a.len, a.batch, (const float*)a.w.data, &a.p, axis, gather, ys, NXSIG_HOST);
  return res_ok(env, &y, rc);
}

/* stft_mel_sharded(group, x_bin, length, batch, window_bin, params, mel_bins, filters_bin, axis) -> {:ok, f32[batch][M][mel_bins], M}
 * (the sharded log-mel: the members' maxima are all-reduced between the two passes) */
static ERL_NIF_TERM nif_stft_mel_sharded(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  grp_res_t* g;
  frames_args_t a;
  int bins, axis;
  const void *x, *f;
  result_t o = {0};
  if (argc != 9 || !get_grp(env, argv[0], &g) || !get_frames_args(env, argv + 2, 0, 0, &a) || !enif_get_int(env, argv[6], &bins) ||
      !enif_get_int(env, argv[8], &axis) || a.p.fft_length < 2 || !get_rows(env, argv[1], NULL, NXSIG_HOST, 4, a.batch, a.len, 1, &x) ||
      !get_rows(env, argv[7], NULL, NXSIG_HOST, 4, bins, a.p.fft_length, 1, &f))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  int rc = res_open(&o, NULL, NXSIG_HOST, 4, (uint64_t)a.batch, (uint64_t)a.out, (uint64_t)bins);
  const float* xs[NXSIG_MAX_MEMBERS] = {(const float*)x};
  float* os[NXSIG_MAX_MEMBERS] = {(float*)o.data};
  if (!rc)
    rc = nxsig_stft_mel_sharded_f32(g->grp, xs, a.len, a.batch, a.len, (const float*)a.w.data, &a.p, bins, (const float*)f, axis, os, NULL, NXSIG_HOST);
  return res_ok2(env, &o, rc, a.out);
}

/* fir_sharded(group, x_bin, length, batch, taps_bin, mode, axis, gather) -> {:ok, y_bin} */
static ERL_NIF_TERM nif_fir_sharded(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  grp_res_t* g;
  fir_args_t a;
  int axis, gather;
  const void* x;
  result_t y = {0};
  if (argc != 8 || !get_grp(env, argv[0], &g) || !get_fir_args(env, argv + 2, 4, &a) || !enif_get_int(env, argv[6], &axis) ||
      !enif_get_int(env, argv[7], &gather) || !get_rows(env, argv[1], NULL, NXSIG_HOST, 4, a.batch, a.len, 1, &x))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  int rc = res_open(&y, NULL, NXSIG_HOST, 4, (uint64_t)a.batch, (uint64_t)a.out, 1);
  const float* xs[NXSIG_MAX_MEMBERS] = {(const float*)x};
  float* ys[NXSIG_MAX_MEMBERS] = {(float*)y.data};
  if (!rc) rc = nxsig_fir_sharded_f32(g->grp, xs, a.len, a.batch, a.len, (const float*)a.h.data, a.taps, a.mode, axis, gather, ys, NXSIG_HOST);
  return res_ok(env, &y, rc);
}

/* ------------------------------------------------------------------------------------------------ device-resident shards
 * NxSignalAMD.Sharded.Tensor: one dense device buffer per group member, the payload never visits the host between
 * group_scatter (Sharded.to_device) and group_gather (Sharded.from_device).  The reference axis being sharded is Nx's
 * vectorized axis (lib/nx_signal.ex:358-363) or, for one long stream, the frame / sample axis. */

/* shard_range(kind, a, b, c, world, rank) -> {x0, x1, y0, y1}
 *   kind 0: nxsig_shard_range(total = a)            -> {begin, end, 0, 0}
 *   kind 1: nxsig_shard_frames(num_frames = a, frame_length = b, hop = c)   -> {m0, m1, s0, s1}
 *   kind 2: nxsig_shard_istft(num_frames = a, frame_length = b, hop = c)    -> {f0, f1, n0, n1}
 *   kind 3: nxsig_shard_fir(length = a, num_taps = b, mode = c)             -> {n0, n1, s0, s1} */
enum { SHARD_RANGE = 0, SHARD_FRAMES = 1, SHARD_ISTFT = 2, SHARD_FIR = 3 };
static int shard_plan(int kind, int64_t a, int32_t b, int32_t c, int world, int rank, int64_t r[4]) {
  switch (kind) {
    case SHARD_RANGE: return nxsig_shard_range(a, world, rank, &r[0], &r[1]);
    case SHARD_FRAMES: return nxsig_shard_frames(a, b, c, world, rank, &r[0], &r[1], &r[2], &r[3]);
    case SHARD_ISTFT: return nxsig_shard_istft(a, b, c, world, rank, &r[0], &r[1], &r[2], &r[3]);
    default: return nxsig_shard_fir(a, b, c, world, rank, &r[0], &r[1], &r[2], &r[3]);
  }
}
static ERL_NIF_TERM nif_shard_range(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  int kind, world, rank;
  ErlNifSInt64 a, b, c;
  if (argc != 6 || !enif_get_int(env, argv[0], &kind) || !enif_get_int64(env, argv[1], &a) || !enif_get_int64(env, argv[2], &b) ||
      !enif_get_int64(env, argv[3], &c) || !enif_get_int(env, argv[4], &world) || !enif_get_int(env, argv[5], &rank))
    return enif_make_badarg(env);
  if (b < -0x7fffffff || b > 0x7fffffff || c < -0x7fffffff || c > 0x7fffffff || kind < SHARD_RANGE || kind > SHARD_FIR) return enif_make_badarg(env);
  int64_t r[4] = {0, 0, 0, 0};
  int rc = shard_plan(kind, a, (int32_t)b, (int32_t)c, world, rank, r);
  if (rc) return mk_error(env, rc);
  return mk_ok(env, enif_make_tuple4(env, enif_make_int64(env, r[0]), enif_make_int64(env, r[1]), enif_make_int64(env, r[2]),
                                     enif_make_int64(env, r[3])));
}

/* [{row0, rows, off_bytes, len_bytes}, ...] — one entry per LOCAL member, in member order */
typedef struct { int64_t row0, rows, off, len; } part_t;
static int get_parts(ErlNifEnv* env, ERL_NIF_TERM list, int n, part_t* out) {
  unsigned len;
  if (!enif_get_list_length(env, list, &len) || (int)len != n) return 0;
  ERL_NIF_TERM head, tail = list;
  for (int i = 0; i < n; ++i) {
    const ERL_NIF_TERM* e;
    int arity;
    ErlNifSInt64 v[4];
    if (!enif_get_list_cell(env, tail, &head, &tail) || !enif_get_tuple(env, head, &arity, &e) || arity != 4) return 0;
    for (int k = 0; k < 4; ++k)
      if (!enif_get_int64(env, e[k], &v[k]) || v[k] < 0) return 0;
    out[i].row0 = v[0]; out[i].rows = v[1]; out[i].off = v[2]; out[i].len = v[3];
  }
  return 1;
}
static int get_bufs(ErlNifEnv* env, ERL_NIF_TERM list, grp_res_t* g, int n, buf_res_t** out) {
  unsigned len;
  if (!enif_get_list_length(env, list, &len) || (int)len != n) return 0;
  ERL_NIF_TERM head, tail = list;
  for (int i = 0; i < n; ++i) {
    if (!enif_get_list_cell(env, tail, &head, &tail) || !get_buf(env, head, &out[i])) return 0;
    if (out[i]->gowner != g || out[i]->member != i) return 0;   /* buffer i must live on member i of THIS group */
  }
  return 1;
}
static ERL_NIF_TERM bufs_to_list(ErlNifEnv* env, grp_res_t* g, int n, void** d, const size_t* bytes) {
  ERL_NIF_TERM t[NXSIG_MAX_MEMBERS];
  for (int i = 0; i < n; ++i) t[i] = make_gbuf(env, g, i, d[i], bytes[i]);
  return enif_make_list_from_array(env, t, (unsigned)n);
}
static void free_members(grp_res_t* g, int n, void** d) {
  for (int i = 0; i < n; ++i)
    if (d[i]) { nxsig_free(nxsig_group_ctx(g->grp, i), d[i]); d[i] = NULL; }
}

/* group_scatter(group, bin, batch, row_bytes, parts) -> {:ok, [buf]}: member i receives rows [row0, row0 + rows) x bytes
 * [off, off + len) of the host tensor [batch][row_bytes], packed densely ([rows][len]) on its own device */
static ERL_NIF_TERM nif_group_scatter(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  grp_res_t* g;
  ErlNifBinary b;
  ErlNifSInt64 batch, row_bytes;
  part_t parts[NXSIG_MAX_MEMBERS];
  if (argc != 5 || !get_grp(env, argv[0], &g) || !enif_inspect_binary(env, argv[1], &b) || !enif_get_int64(env, argv[2], &batch) ||
      !enif_get_int64(env, argv[3], &row_bytes))
    return enif_make_badarg(env);
  const int n = nxsig_group_local_count(g->grp);
  if (n < 1 || n > NXSIG_MAX_MEMBERS || batch < 1 || row_bytes < 1 || (uint64_t)b.size / (uint64_t)batch != (uint64_t)row_bytes ||
      b.size % (size_t)batch || !get_parts(env, argv[4], n, parts))
    return enif_make_badarg(env);
  for (int i = 0; i < n; ++i)
    if (parts[i].row0 > batch || parts[i].rows > batch - parts[i].row0 || parts[i].off > row_bytes || parts[i].len > row_bytes - parts[i].off)
      return enif_make_badarg(env);   /* compared without adding: the four values come from Erlang and may sum past INT64_MAX */
  void* d[NXSIG_MAX_MEMBERS] = {0};
  size_t bytes[NXSIG_MAX_MEMBERS];
  for (int i = 0; i < n; ++i) {
    nxsig_ctx* c = nxsig_group_ctx(g->grp, i);
    bytes[i] = (size_t)parts[i].rows * (size_t)parts[i].len;
    int rc = nxsig_alloc(c, bytes[i] ? bytes[i] : 4, &d[i]);
    for (int64_t r = 0; !rc && r < parts[i].rows && parts[i].len > 0; ++r)
      rc = nxsig_upload(c, (char*)d[i] + (size_t)r * (size_t)parts[i].len,
                        b.data + (size_t)(parts[i].row0 + r) * (size_t)row_bytes + (size_t)parts[i].off, (size_t)parts[i].len);
    if (rc) { free_members(g, n, d); return mk_error(env, rc); }
  }
  return mk_ok(env, bufs_to_list(env, g, n, d, bytes));
}

/* group_gather(group, [buf], batch, row_bytes, parts) -> {:ok, bin}: the inverse of group_scatter for RESULT shards */
static ERL_NIF_TERM nif_group_gather(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  grp_res_t* g;
  ErlNifSInt64 batch, row_bytes;
  part_t parts[NXSIG_MAX_MEMBERS];
  buf_res_t* bufs[NXSIG_MAX_MEMBERS];
  result_t o = {0};
  if (argc != 5 || !get_grp(env, argv[0], &g) || !enif_get_int64(env, argv[2], &batch) || !enif_get_int64(env, argv[3], &row_bytes))
    return enif_make_badarg(env);
  const int n = nxsig_group_local_count(g->grp);
  if (n < 1 || n > NXSIG_MAX_MEMBERS || batch < 1 || row_bytes < 1 || !get_bufs(env, argv[1], g, n, bufs) || !get_parts(env, argv[4], n, parts))
    return enif_make_badarg(env);
  for (int i = 0; i < n; ++i)
    if (parts[i].row0 > batch || parts[i].rows > batch - parts[i].row0 || parts[i].off > row_bytes || parts[i].len > row_bytes - parts[i].off ||
        (parts[i].len > 0 && (uint64_t)parts[i].rows > (uint64_t)bufs[i]->bytes / (uint64_t)parts[i].len))
      return enif_make_badarg(env);
  int rc = res_open(&o, NULL, NXSIG_HOST, 1, (uint64_t)batch, (uint64_t)row_bytes, 1);
  if (!rc) memset(o.data, 0, o.bytes);   /* positions no shard covers (none for the plans of nxsig_shard_*) read as zero */
  for (int i = 0; !rc && i < n; ++i) {
    nxsig_ctx* c = nxsig_group_ctx(g->grp, i);
    rc = nxsig_sync(c);          /* the shard may still be in flight on the member's stream */
    for (int64_t r = 0; !rc && r < parts[i].rows && parts[i].len > 0; ++r)
      rc = nxsig_download(c, (char*)o.data + (size_t)(parts[i].row0 + r) * (size_t)row_bytes + (size_t)parts[i].off,
                          (const char*)bufs[i]->dptr + (size_t)r * (size_t)parts[i].len, (size_t)parts[i].len);
  }
  return res_ok(env, &o, rc);
}

/* The member buffers of a *_sharded_dev call and the result shards it allocates.  Shard sizes (bytes per member) follow the partition
 * rules of the library: the channels axis splits the `batch` rows (nxsig_shard_range), any other axis splits every row by the plan of
 * `kind` — SHARD_FRAMES stft (f32 samples in, frames out; a = num_frames, b = frame_length, c = hop), SHARD_ISTFT (frames in, samples
 * out; the same a, b, c), SHARD_FIR (samples in, samples out; a = length, b = taps, c = mode).  Each plan answers {x0, x1, y0, y1}: the
 * frames / fir plans give the OUTPUT range first and the input span second, the istft plan the input frames first. */
typedef struct {
  int n;
  buf_res_t* in[NXSIG_MAX_MEMBERS];
  void* out[NXSIG_MAX_MEMBERS];
  size_t bytes[NXSIG_MAX_MEMBERS];
} shards_t;
static int get_shards(ErlNifEnv* env, ERL_NIF_TERM list, grp_res_t* g, shards_t* s) {
  memset(s->out, 0, sizeof s->out);
  s->n = nxsig_group_local_count(g->grp);
  return s->n >= 1 && s->n <= NXSIG_MAX_MEMBERS && get_bufs(env, list, g, s->n, s->in);
}
/* bytes per member of the input (output = 0) or output (1) shards; gather: every member holds the whole output tensor */
static int shard_sizes(grp_res_t* g, int n, int output, int axis, int gather, int64_t batch, int64_t items_per_row, int64_t item_bytes, int kind,
                       int64_t a, int32_t b, int32_t c, size_t* bytes) {
  const int world = nxsig_group_world(g->grp);
  const int lo = (kind == SHARD_ISTFT) == output ? 2 : 0;   /* which pair of the plan's answer this side of the call reads */
  for (int i = 0; i < n; ++i) {
    const int rank = nxsig_group_rank(g->grp, i);
    int64_t rows = batch, items = items_per_row, r[4];
    int rc;
    if (!gather && axis == NXSIG_SHARD_CHANNELS) { if ((rc = shard_plan(SHARD_RANGE, batch, 0, 0, world, rank, r))) return rc; rows = r[1] - r[0]; }
    else if (!gather) { if ((rc = shard_plan(kind, a, b, c, world, rank, r))) return rc; items = r[lo + 1] - r[lo]; }
    size_t sz = (size_t)item_bytes;
    if (rows < 0 || items < 0 || !mul_size(&sz, (uint64_t)rows) || !mul_size(&sz, (uint64_t)items)) return NXSIG_ERR_OOM;
    bytes[i] = sz;
  }
  return 0;
}
/* What the four *_sharded_dev NIFs do between reading their terms and calling the library: refuse member buffers smaller than the
 * shards the call will READ — they would be read out of bounds on the device, e.g. a shard scattered for another plan, or
 * the frame shards of stft(axis: :frames) handed to istft, which needs halo frames too — then allocate the result shards.
 * Returns 0 with s->out / s->bytes filled, or the error term in *err. */
static int shards_open(ErlNifEnv* env, grp_res_t* g, shards_t* s, int axis, int gather, int64_t batch, int64_t in_items, int64_t in_item_bytes,
                       int64_t out_items, int64_t out_item_bytes, int kind, int64_t a, int32_t b, int32_t c, ERL_NIF_TERM* err) {
  int rc = shard_sizes(g, s->n, 0, axis, 0, batch, in_items, in_item_bytes, kind, a, b, c, s->bytes);
  for (int i = 0; !rc && i < s->n; ++i)
    if (s->in[i]->bytes < s->bytes[i]) { *err = enif_make_badarg(env); return 1; }
  if (!rc) rc = shard_sizes(g, s->n, 1, axis, gather, batch, out_items, out_item_bytes, kind, a, b, c, s->bytes);
  if (rc) { *err = rc == NXSIG_ERR_OOM ? mk_oom(env) : mk_error(env, rc); return 1; }
  for (int i = 0; i < s->n; ++i)
    if ((rc = nxsig_alloc(nxsig_group_ctx(g->grp, i), s->bytes[i] ? s->bytes[i] : 4, &s->out[i]))) {
      free_members(g, s->n, s->out);
      *err = mk_error(env, rc);
      return 1;
    }
  return 0;
}
/* the error of a failed library call, once the result shards are returned */
static ERL_NIF_TERM shards_fail(ErlNifEnv* env, grp_res_t* g, shards_t* s, int rc) {
  free_members(g, s->n, s->out);
  return mk_error(env, rc);
}

/* stft_sharded_dev(group, [x_buf], length, batch, window_bin, params, axis, gather) -> {:ok, [z_buf], num_frames}
 * x_buf i = member i's dense input shard (rows [c0, c1) of the tensor / the span [s0, s1) of every row); the result shards
 * (or, gather = 1, the whole c64[batch][M][K] on every member, assembled by the RCCL all-gather) stay on their devices */
static ERL_NIF_TERM nif_stft_sharded_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  grp_res_t* g;
  frames_args_t a;
  int axis, gather;
  shards_t s;
  ERL_NIF_TERM err;
  if (argc != 8 || !get_grp(env, argv[0], &g) || !get_frames_args(env, argv + 2, 0, 0, &a) || !enif_get_int(env, argv[6], &axis) ||
      !enif_get_int(env, argv[7], &gather) || !get_shards(env, argv[1], g, &s))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  if (shards_open(env, g, &s, axis, gather, a.batch, a.len, 4, a.out, (int64_t)a.p.fft_length * 8, SHARD_FRAMES, a.out, a.p.frame_length, a.p.hop, &err))
    return err;
  const float* xs[NXSIG_MAX_MEMBERS];
  nxsig_c64* zs[NXSIG_MAX_MEMBERS];
  for (int i = 0; i < s.n; ++i) { xs[i] = (const float*)s.in[i]->dptr; zs[i] = (nxsig_c64*)s.out[i]; }
  /* channel shards: rows of the full length; frame shards: dense per-member spans (batch_stride 0, see nxsig.h) */
  int rc = nxsig_stft_sharded_f32(g->grp, xs, a.len, a.batch, axis == NXSIG_SHARD_CHANNELS ? a.len : 0, (const float*)a.w.data, &a.p, axis, gather,
                                  zs, NXSIG_DEVICE);
  if (rc) return shards_fail(env, g, &s, rc);
  return mk_ok2(env, bufs_to_list(env, g, s.n, s.out, s.bytes), enif_make_int64(env, a.out));
}

/* istft_sharded_dev(group, [z_buf], num_frames, batch, window_bin, params, axis, gather) -> {:ok, [y_buf]} */
static ERL_NIF_TERM nif_istft_sharded_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  grp_res_t* g;
  frames_args_t a;
  int axis, gather;
  shards_t s;
  ERL_NIF_TERM err;
  if (argc != 8 || !get_grp(env, argv[0], &g) || !get_frames_args(env, argv + 2, 0, 1, &a) || !enif_get_int(env, argv[6], &axis) ||
      !enif_get_int(env, argv[7], &gather) || !get_shards(env, argv[1], g, &s))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  if (shards_open(env, g, &s, axis, gather, a.batch, a.len, (int64_t)a.p.frame_length * 8, a.out, 8, SHARD_ISTFT, a.len, a.p.frame_length, a.p.hop, &err))
    return err;
  const nxsig_c64* zs[NXSIG_MAX_MEMBERS];
  nxsig_c64* ys[NXSIG_MAX_MEMBERS];
  for (int i = 0; i < s.n; ++i) { zs[i] = (const nxsig_c64*)s.in[i]->dptr; ys[i] = (nxsig_c64*)s.out[i]; }
  int rc = nxsig_istft_sharded_c64(g->grp, zs, a.len, a.batch, (const float*)a.w.data, &a.p, axis, gather, ys, NXSIG_DEVICE);
  if (rc) return shards_fail(env, g, &s, rc);
  return mk_ok(env, bufs_to_list(env, g, s.n, s.out, s.bytes));
}

/* fir_sharded_dev(group, [x_buf], length, batch, taps_bin, mode, axis, gather) -> {:ok, [y_buf]} */
static ERL_NIF_TERM nif_fir_sharded_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  grp_res_t* g;
  fir_args_t a;
  int axis, gather;
  shards_t s;
  ERL_NIF_TERM err;
  if (argc != 8 || !get_grp(env, argv[0], &g) || !get_fir_args(env, argv + 2, 4, &a) || !enif_get_int(env, argv[6], &axis) ||
      !enif_get_int(env, argv[7], &gather) || !get_shards(env, argv[1], g, &s))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  if (shards_open(env, g, &s, axis, gather, a.batch, a.len, 4, a.out, 4, SHARD_FIR, a.len, a.taps, a.mode, &err)) return err;
  const float* xs[NXSIG_MAX_MEMBERS];
  float* ys[NXSIG_MAX_MEMBERS];
  for (int i = 0; i < s.n; ++i) { xs[i] = (const float*)s.in[i]->dptr; ys[i] = (float*)s.out[i]; }
  int rc = nxsig_fir_sharded_f32(g->grp, xs, a.len, a.batch, axis == NXSIG_SHARD_CHANNELS ? a.len : 0, (const float*)a.h.data, a.taps, a.mode, axis,
                                 gather, ys, NXSIG_DEVICE);
  if (rc) return shards_fail(env, g, &s, rc);
  return mk_ok(env, bufs_to_list(env, g, s.n, s.out, s.bytes));
}

/* stft_mel_sharded_dev(group, [x_buf], length, batch, window_bin, params, mel_bins, filters_bin, axis) -> {:ok, [o_buf], M} */
static ERL_NIF_TERM nif_stft_mel_sharded_dev(ErlNifEnv* env, int argc, const ERL_NIF_TERM argv[]) {
  grp_res_t* g;
  frames_args_t a;
  int bins, axis;
  const void* f;
  shards_t s;
  ERL_NIF_TERM err;
  if (argc != 9 || !get_grp(env, argv[0], &g) || !get_frames_args(env, argv + 2, 0, 0, &a) || !enif_get_int(env, argv[6], &bins) ||
      !enif_get_int(env, argv[8], &axis) || a.p.fft_length < 2 || !get_rows(env, argv[7], NULL, NXSIG_HOST, 4, bins, a.p.fft_length, 1, &f) ||
      !get_shards(env, argv[1], g, &s))
    return enif_make_badarg(env);
  if (a.out < 0) return mk_error(env, (int)a.out);
  if (shards_open(env, g, &s, axis, 0, a.batch, a.len, 4, a.out, (int64_t)bins * 4, SHARD_FRAMES, a.out, a.p.frame_length, a.p.hop, &err)) return err;
  const float* xs[NXSIG_MAX_MEMBERS];
  float* os[NXSIG_MAX_MEMBERS];
  for (int i = 0; i < s.n; ++i) { xs[i] = (const float*)s.in[i]->dptr; os[i] = (float*)s.out[i]; }
  int rc = nxsig_stft_mel_sharded_f32(g->grp, xs, a.len, a.batch, axis == NXSIG_SHARD_CHANNELS ? a.len : 0, (const float*)a.w.data, &a.p, bins,
                                      (const float*)f, axis, os, NULL, NXSIG_DEVICE);
  if (rc) return shards_fail(env, g, &s, rc);
  return mk_ok2(env, bufs_to_list(env, g, s.n, s.out, s.bytes), enif_make_int64(env, a.out));
}

static int load(ErlNifEnv* env, void** priv, ERL_NIF_TERM info) {
  (void)priv; (void)info;
  CTX_RES = enif_open_resource_type(env, NULL, "nxsig_ctx", ctx_dtor, ERL_NIF_RT_CREATE | ERL_NIF_RT_TAKEOVER, NULL);
  BUF_RES = enif_open_resource_type(env, NULL, "nxsig_buf", buf_dtor, ERL_NIF_RT_CREATE | ERL_NIF_RT_TAKEOVER, NULL);
  GRP_RES = enif_open_resource_type(env, NULL, "nxsig_group", grp_dtor, ERL_NIF_RT_CREATE | ERL_NIF_RT_TAKEOVER, NULL);
  return (CTX_RES && BUF_RES && GRP_RES) ? 0 : -1;
}
static int upgrade(ErlNifEnv* env, void** priv, void** old, ERL_NIF_TERM info) { (void)old; return load(env, priv, info); }

static ErlNifFunc funcs[] = {
    {"device_count", 0, nif_device_count, 0},
    {"ctx_create", 1, nif_ctx_create, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"sync", 1, nif_sync, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"last_dispatch", 1, nif_last_dispatch, ERL_NIF_DIRTY_JOB_IO_BOUND},   /* takes the context mutex: may wait behind a running call */
    {"window", 5, nif_window, 0},
    {"firwin", 7, nif_firwin, 0},
    {"fft_frequencies", 3, nif_fft_frequencies, 0},
    {"mel_filters", 5, nif_mel_filters, ERL_NIF_DIRTY_JOB_CPU_BOUND},
    {"sinc", 1, nif_sinc, 0},
    {"stft", 6, nif_stft, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"stft_c64", 6, nif_stft_c64, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"istft", 6, nif_istft, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"istft_filtered", 7, nif_istft_filtered, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"fir", 6, nif_fir, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"as_windowed", 9, nif_as_windowed, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"overlap_and_add", 7, nif_overlap_and_add, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"fft", 7, nif_fft, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"fftconvolve_c64", 4, nif_fftconvolve_c64, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"fft_nd", 7, nif_fft_nd, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"fftconvolve_nd", 8, nif_fftconvolve_nd, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"convolve_direct", 8, nif_convolve_direct, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"median", 5, nif_median, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"wiener", 7, nif_wiener, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"resample_poly", 8, nif_resample_poly, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"resample_poly_dev", 8, nif_resample_poly_dev, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"welch", 10, nif_welch, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"csd", 11, nif_csd, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"argrelextrema", 7, nif_argrelextrema, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"nonzero", 3, nif_nonzero, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"sawtooth", 4, nif_sawtooth, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"square", 5, nif_square, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"gaussian_pulse", 6, nif_gaussian_pulse, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"chirp", 7, nif_chirp, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"polynomial_sweep", 6, nif_polynomial_sweep, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"unit_impulse", 4, nif_unit_impulse, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"stft_to_mel", 6, nif_stft_to_mel, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"stft_mel", 8, nif_stft_mel, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"stft_magnitude", 7, nif_stft_magnitude, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"to_device", 2, nif_to_device, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"from_device", 1, nif_from_device, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"buf_size", 1, nif_buf_size, 0},
    {"stft_dev", 6, nif_stft_dev, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"stft_c64_dev", 6, nif_stft_c64_dev, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"stft_onesided_dev", 6, nif_stft_onesided_dev, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"stft_packed_dev", 6, nif_stft_packed_dev, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"istft_packed_dev", 6, nif_istft_packed_dev, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"istft_dev", 6, nif_istft_dev, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"istft_filtered_dev", 7, nif_istft_filtered_dev, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"fir_dev", 6, nif_fir_dev, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"spectrum_mul_dev", 5, nif_spectrum_mul_dev, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"spectrum_mask", 8, nif_spectrum_mask, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"istft_masked", 9, nif_istft_masked, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"group_create", 1, nif_group_create, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"group_info", 1, nif_group_info, 0},
    {"stft_sharded", 8, nif_stft_sharded, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"istft_sharded", 8, nif_istft_sharded, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"fir_sharded", 8, nif_fir_sharded, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"stft_mel_sharded", 9, nif_stft_mel_sharded, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"shard_range", 6, nif_shard_range, 0},
    {"group_scatter", 5, nif_group_scatter, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"group_gather", 5, nif_group_gather, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"stft_sharded_dev", 8, nif_stft_sharded_dev, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"istft_sharded_dev", 8, nif_istft_sharded_dev, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"fir_sharded_dev", 8, nif_fir_sharded_dev, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"stft_mel_sharded_dev", 9, nif_stft_mel_sharded_dev, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"window_f64", 5, nif_window_f64, 0},
    {"firwin_f64", 7, nif_firwin_f64, 0},
    {"fft_frequencies_f64", 3, nif_fft_frequencies_f64, 0},
    {"sinc_f64", 1, nif_sinc_f64, 0},
    {"stft_f64", 7, nif_stft_f64, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"stft_c128", 7, nif_stft_c128, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"istft_c128", 7, nif_istft_c128, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"fir_f64", 6, nif_fir_f64, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"fft_c128", 7, nif_fft_c128, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"as_windowed_f64", 9, nif_as_windowed_f64, ERL_NIF_DIRTY_JOB_IO_BOUND},
    {"overlap_and_add_f64", 7, nif_overlap_and_add_f64, ERL_NIF_DIRTY_JOB_IO_BOUND},
};

ERL_NIF_INIT(Elixir.NxSignalAMD.NIF, funcs, load, NULL, upgrade, NULL)
