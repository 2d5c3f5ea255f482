"""TEST INFRASTRUCTURE: the dirty-NIF shim over a RECORDING stand-in for libnxsig (no GPU).

`build()` compiles nif/nxsig_nif.c and tests/stub/erl_nif_fake.c exactly as nif_harness.build() does, but links them with
tests/stub/nxsig_recorder.c and one generated definition per nxsig_* function the shim calls into tests/_nif_trace.so.  The
definitions are written from the prototypes of include/nxsig.h (`generate()`): a function without a context or group parameter
is forwarded to the real libnxsig.so through dlopen / dlsym, every other one writes its arguments to the recorder's log and
returns 0.  `lib()` loads the result next to (not instead of) nif_harness's own library; `session()` points nif_harness at it
for the length of a `with` block, so that H.call / H.Res drive the traced shim."""
import contextlib
import ctypes as C
import os
import re
import subprocess

import nif_harness as H

ROOT = H.ROOT
SO = os.path.join(ROOT, "tests", "_nif_trace.so")
HEADER = os.path.join(ROOT, "include", "nxsig.h")
RECORDER = os.path.join(ROOT, "tests", "stub", "nxsig_recorder.c")
REAL = os.path.join(ROOT, "nx_signal_amd", "libnxsig.so")
HANDWRITTEN = {"nxsig_ctx_create", "nxsig_ctx_destroy", "nxsig_group_create_local", "nxsig_group_destroy", "nxsig_group_ctx",
               "nxsig_group_world", "nxsig_group_local_count", "nxsig_group_rank", "nxsig_alloc", "nxsig_free", "nxsig_last_error"}
# arrays whose length is another parameter of the same function: recorded by value
COUNTED = {"shape": "rank", "a_shape": "rank", "b_shape": "rank", "axes": "n_axes", "lengths": "n_axes", "kernel_shape": "rank",
           "kernel_size": "rank", "cutoff": "n_cutoff", "coefs": "ncoefs", "index": "rank"}
GPU_WITHOUT_CTX = {"nxsig_device_count"}   # asks the HIP runtime although it takes no context: recorded, never forwarded
_INTS = {"int", "int32_t", "int64_t", "uint32_t", "size_t"}


def prototypes():
    """{name: (return type, [(type, name)])} of every `ret nxsig_name(args);` in include/nxsig.h"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"(?:^|[;}])\s*((?:const\s+)?\w+\s*\**)\s*(nxsig_\w+)\s*\(([^()]*)\)\s*;", text, re.M):
        params = []
        for p in (q.strip() for q in m.group(3).split(",")):
            if p != "void":
                t, n = re.match(r"(.*?)(\w+)$", p, re.S).groups()
                params.append((re.sub(r"\s*\*\s*", "*", " ".join(t.split())), n))
        out[m.group(2)] = (" ".join(m.group(1).split()), params)
    return out


def shim_calls():
    """the nxsig_* functions nif/nxsig_nif.c calls"""
    text = re.sub(r"/\*.*?\*/", " ", open(H.SRC[0]).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(nxsig_[a-z0-9_]+)\s*[(,)]", text)) & set(prototypes()))


def forwarded(name, params):
    return name not in GPU_WITHOUT_CTX and not any("nxsig_ctx" in t or "nxsig_group" in t for t, _ in params)


def _definition(name, ret, params):
    sig = ", ".join(f"{t} {n}" for t, n in params) or "void"
    args = ", ".join(n for _, n in params)
    if forwarded(name, params):
        body = [f"  typedef {ret} (*fn_t)({', '.join(t for t, _ in params) or 'void'});", "  static fn_t fn;"]
        if ret in _INTS:
            body.append(f'  int code; if (fail_hit("{name}", &code)) return code;')
        body += [f'  if (!fn) fn = (fn_t)real("{name}");', "  g_injected = 0;", f"  return fn({args});"]
        return f"{ret} {name}({sig}) {{\n" + "\n".join(body) + "\n}\n"
    names = {n for _, n in params}
    body, after = [f'  put("{name}(");'], []
    for i, (t, n) in enumerate(params):
        sep = '  put(",");' if i else ""
        if t == "nxsig_ctx*":
            put = f"put_ctx({n});"
        elif "nxsig_group*" in t:
            put = f'put({n} ? "grp" : "null");'
        elif t == "const nxsig_stft_params*":
            put = f"put_params({n});"
        elif t in _INTS:
            put = f'put("%lld", (long long){n});'
        elif t == "double":
            put = f'put("%.17g", {n});'
        elif t.endswith("*const*"):   # one pointer per local member; a host call only has element 0
            put = f"put_ptrs((const void* const*){n}, mem == NXSIG_DEVICE ? g->n : 1);"
        elif n in COUNTED and COUNTED[n] in names and t in ("const int64_t*", "const int32_t*", "const double*"):
            put = f"put_{ {'const int64_t*': 'i64s', 'const int32_t*': 'i32s', 'const double*': 'f64s'}[t]}({n}, {COUNTED[n]});"
        elif t == "char*":
            put = f"put_ptr({n});"
            after.append(f"  fill_text({n}, buflen);")
        elif t.endswith("*"):
            put = f"put_ptr({n});"
            if n == "out_shape":
                after.append(f"  fill_conv_shape(a_shape, b_shape, rank, mode, {n});")
        else:
            raise ValueError(f"{name}: no rule for parameter `{t} {n}`")
        body.append(f"{sep}  {put}")
    assert ret in _INTS, (name, ret)
    body += after + [f'  return recorded("{name}");']
    return f"{ret} {name}({sig}) {{\n" + "\n".join(body) + "\n}\n"


def generate():
    """the generated half of the stand-in: C text"""
    protos = prototypes()
    return "".join(_definition(n, *protos[n]) for n in shim_calls() if n not in HANDWRITTEN)


def build(force=False):
    deps = H.SRC + [RECORDER, HEADER, os.path.join(ROOT, "tests", "stub", "erl_nif.h"), os.path.abspath(__file__)]
    if not force and os.path.exists(SO) and all(os.path.getmtime(SO) >= os.path.getmtime(d) for d in deps):
        return SO
    cmd = ["gcc", "-std=c11", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-D_GNU_SOURCE",
           "-I" + os.path.join(ROOT, "tests", "stub"), *H.SRC, "-x", "c", "-", "-o", SO, "-Wl,-Bsymbolic", "-ldl"]
    subprocess.run(cmd, input=f'#include "{RECORDER}"\n{generate()}'.encode(), check=True)
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = H.open_lib(build())
        for name, res, args in [("rec_log", C.c_char_p, []), ("rec_reset", None, []), ("rec_live_allocs", C.c_long, []),
                                ("rec_fail_next", None, [C.c_char_p, C.c_int, C.c_int]), ("rec_open_real", C.c_int, [C.c_char_p])]:
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        assert L.rec_open_real(REAL.encode()), REAL
        _lib = L
    return _lib


@contextlib.contextmanager
def session():
    """nif_harness drives the traced shim inside the block; every H.Res made inside must be released inside"""
    saved = H._lib, H._keep
    H._lib, H._keep = lib(), None
    try:
        yield H._lib
    finally:
        H._lib, H._keep = saved
