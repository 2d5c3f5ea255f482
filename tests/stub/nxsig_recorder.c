/*
 * TEST INFRASTRUCTURE ONLY — the hand-written half of a recording stand-in for libnxsig (tests/nif_trace.py).
 *
 * tests/nif_trace.py reads the prototypes of include/nxsig.h, writes one definition per nxsig_* function the shim calls after
 * this file and compiles the two as one translation unit next to nif/nxsig_nif.c and tests/stub/erl_nif_fake.c.  A function
 * that takes no context and no group (host generators, length helpers, shard plans) goes to the real library, opened with
 * dlopen(RTLD_LOCAL) and called through a pointer of its own type.  Every other function appends one line to the log
 *     nxsig_fir_f32(ctx,host,40,2,40,host,5,1,dev#0,1)
 * — integers and doubles by value, nxsig_stft_params by field, counted arrays by value, every other pointer as null / host /
 * dev#k (+offset), k the position among the live blocks of nxsig_alloc — and returns 0 without touching its outputs (the few
 * outputs the shim reads back are filled with fixed values, see below).  rec_fail_next() makes one later call of a named
 * function return a code instead: that is how a test reaches a NIF's clean-up path.
 */
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/nxsig.h"

struct nxsig_ctx { int member; };                              /* -1: a context of its own; i: member i of a group */
struct nxsig_group { int n; nxsig_ctx members[64]; };

/* ---- the log ---- */
static char* g_log;
static size_t g_len, g_cap;
static void put(const char* fmt, ...) {
  va_list ap;
  if (g_cap - g_len < 512) { g_cap = g_cap ? g_cap * 2 : 1 << 16; g_log = (char*)realloc(g_log, g_cap); }
  va_start(ap, fmt);
  g_len += (size_t)vsnprintf(g_log + g_len, 512, fmt, ap);
  va_end(ap);
}
const char* rec_log(void) { return g_len ? g_log : ""; }
void rec_reset(void) { g_len = 0; }

/* ---- live device blocks ---- */
static struct { char* p; size_t n; } g_blocks[256];
static int g_nblocks;
long rec_live_allocs(void) { return g_nblocks; }

static void put_ptr(const void* p) {
  if (!p) { put("null"); return; }
  for (int k = 0; k < g_nblocks; ++k)
    if ((const char*)p >= g_blocks[k].p && (const char*)p < g_blocks[k].p + g_blocks[k].n) {
      put("dev#%d", k);
      if ((const char*)p != g_blocks[k].p) put("+%ld", (long)((const char*)p - g_blocks[k].p));
      return;
    }
  put("host");
}
static void put_ctx(const nxsig_ctx* c) {
  if (!c) put("null");
  else if (c->member < 0) put("ctx");
  else put("ctx#%d", c->member);
}
static void put_params(const nxsig_stft_params* p) {
  if (!p) { put("null"); return; }
  put("{%d,%d,%d,%d,%lld,%lld,%d,%.17g}", p->frame_length, p->hop, p->fft_length, p->pad_mode, (long long)p->pad_lo, (long long)p->pad_hi,
      p->scaling, p->sampling_rate);
}
#define PUT_ARRAY(name, type, fmt, cast)                                          \
  static void name(const type* v, long long n) {                                  \
    if (!v) { put("null"); return; }                                              \
    put("[");                                                                     \
    if (n < 0 || n > 64) put("?%lld", n);                                         \
    else for (long long i = 0; i < n; ++i) put(i ? " " fmt : fmt, (cast)v[i]);    \
    put("]");                                                                     \
  }
PUT_ARRAY(put_i64s, int64_t, "%lld", long long)
PUT_ARRAY(put_i32s, int32_t, "%d", int)
PUT_ARRAY(put_f64s, double, "%.17g", double)
static void put_ptrs(const void* const* v, int n) {
  put("[");
  for (int i = 0; i < n; ++i) { if (i) put(" "); put_ptr(v[i]); }
  put("]");
}

/* ---- the switch: the (skip + 1)-th next call of `name` returns `code` ---- */
static char g_fail_name[64];
static int g_fail_code, g_fail_skip, g_injected;
void rec_fail_next(const char* name, int code, int skip) {
  snprintf(g_fail_name, sizeof g_fail_name, "%s", name ? name : "");
  g_fail_code = code; g_fail_skip = skip;
}
static int fail_hit(const char* name, int* code) {
  if (!g_fail_name[0] || strcmp(name, g_fail_name) || g_fail_skip-- > 0) return 0;
  g_fail_name[0] = 0; g_injected = 1; *code = g_fail_code;
  return 1;
}
/* a recorded call ends its line here */
static int recorded(const char* name) {
  int code = 0;
  if (fail_hit(name, &code)) put(")!%d\n", code);
  else put(")\n");
  return code;
}

/* ---- the real library behind the functions that need no GPU ---- */
static void* g_real;
int rec_open_real(const char* path) { g_real = dlopen(path, RTLD_NOW | RTLD_LOCAL); return g_real != NULL; }
static void* real(const char* name) {
  void* f = g_real ? dlsym(g_real, name) : NULL;
  if (!f) { fprintf(stderr, "nxsig_recorder: %s not found in the real library\n", name); abort(); }
  return f;
}
const char* nxsig_last_error(void) {
  typedef const char* (*fn_t)(void);
  static fn_t fn;
  if (g_injected) return "injected failure";
  if (!fn) fn = (fn_t)real("nxsig_last_error");
  return fn();
}

/* ---- the outputs the shim reads back ---- */
static void fill_text(char* buf, size_t buflen) { if (buf && buflen) snprintf(buf, buflen, "%s", "recorded"); }
static void fill_conv_shape(const int64_t* a, const int64_t* b, int32_t rank, int32_t mode, int64_t* out) {
  for (int d = 0; out && d < rank; ++d)
    out[d] = mode == NXSIG_CONV_FULL ? a[d] + b[d] - 1 : mode == NXSIG_CONV_SAME ? a[d] : (a[d] > b[d] ? a[d] - b[d] : b[d] - a[d]) + 1;
}

/* ---- handles and memory ---- */
int nxsig_ctx_create(int device, nxsig_ctx** out) {
  put("nxsig_ctx_create(%d", device);
  int rc = recorded("nxsig_ctx_create");
  if (rc) return rc;
  *out = (nxsig_ctx*)malloc(sizeof **out);
  (*out)->member = -1;
  return 0;
}
void nxsig_ctx_destroy(nxsig_ctx* ctx) { put("nxsig_ctx_destroy("); put_ctx(ctx); put(")\n"); free(ctx); }
int nxsig_group_create_local(int32_t n, const int32_t* device_ids, nxsig_group** out) {
  put("nxsig_group_create_local(%d,", n); put_i32s(device_ids, n);
  int rc = recorded("nxsig_group_create_local");
  if (rc) return rc;
  *out = (nxsig_group*)calloc(1, sizeof **out);
  (*out)->n = n;
  for (int i = 0; i < 64; ++i) (*out)->members[i].member = i;
  return 0;
}
void nxsig_group_destroy(nxsig_group* g) { put("nxsig_group_destroy(grp)\n"); free(g); }
nxsig_ctx* nxsig_group_ctx(nxsig_group* g, int32_t i) { return i >= 0 && i < g->n ? &g->members[i] : NULL; }
int32_t nxsig_group_world(const nxsig_group* g) { return g->n; }
int32_t nxsig_group_local_count(const nxsig_group* g) { return g->n; }
int32_t nxsig_group_rank(const nxsig_group* g, int32_t i) { (void)g; return i; }
int nxsig_alloc(nxsig_ctx* ctx, size_t bytes, void** dptr) {
  put("nxsig_alloc("); put_ctx(ctx); put(",%lld", (long long)bytes);
  int rc = recorded("nxsig_alloc");
  if (rc) return rc;
  if (g_nblocks == 256) abort();
  g_blocks[g_nblocks].p = (char*)malloc(bytes ? bytes : 1);
  g_blocks[g_nblocks].n = bytes ? bytes : 1;
  *dptr = g_blocks[g_nblocks++].p;
  return 0;
}
int nxsig_free(nxsig_ctx* ctx, void* dptr) {
  put("nxsig_free("); put_ctx(ctx); put(","); put_ptr(dptr); put(")\n");
  for (int k = 0; k < g_nblocks; ++k)
    if (g_blocks[k].p == (char*)dptr) {
      free(dptr);
      memmove(&g_blocks[k], &g_blocks[k + 1], sizeof g_blocks[0] * (size_t)(g_nblocks - k - 1));
      --g_nblocks;
      break;
    }
  return 0;
}

/* ---- the definitions tests/nif_trace.py generates from include/nxsig.h follow ---- */
