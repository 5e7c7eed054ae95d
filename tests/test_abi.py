"""CPU-side checks of the C ABI: the library loads without a GPU and exports every symbol
include/dvm.h declares; the ctypes table covers the header one to one."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "dvm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dvm_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_something():
    syms = header_symbols()
    assert "dvm_softcorr_fwd_f32" in syms and "dvm_pair_direction_fwd_f32" in syms and len(syms) >= 15


def test_library_exports_every_declared_symbol():
    from dvm import _lib
    assert os.path.exists(_lib.SO_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_lib.SO_PATH)
    for s in header_symbols():
        assert hasattr(lib, s), "libdvm_hip.so does not export %s" % s


def test_ctypes_table_matches_header():
    from dvm import _lib
    assert sorted(_lib.SIGNATURES) == header_symbols()


HEADER_FORMS = """
/* a declaration inside a comment:
 * int dvm_in_a_comment(int x);
 */
#ifndef DVM_SAMPLE_H
#define DVM_SAMPLE_VERSION 1
extern "C" {
typedef int (*dvm_callback_fn)(void *user, void *buf, size_t count, void *stream);
typedef struct dvm_thing {
    dvm_callback_fn call;
    void *user;
} dvm_thing;
// int dvm_in_a_line_comment(void);
int dvm_multi_line(const float *x, int B, float slope,
                   int32_t *idx /* may be NULL */, void *ws,
                   size_t ws_bytes,
                   void *stream);
size_t dvm_scalars(long R, size_t n, unsigned mask, unsigned int mask2, double scale, double *out);
int dvm_tables(const float *const *rows, const dvm_thing *thing, const double *w, int);
const char *dvm_text(void);
int dvm_no_arguments();
}
#endif
"""


def test_header_parser_forms():
    """Every form of declaration the header may use, on a literal header: the exact tuples, and no default for a type the parser
    does not know."""
    from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_uint, c_void_p as P
    from dvm import _lib
    got = _lib.parse_header(HEADER_FORMS)
    assert got == {
        "dvm_multi_line": (c_int, [P, c_int, c_float, P, P, c_size_t, P]),
        "dvm_scalars": (c_size_t, [c_long, c_size_t, c_uint, c_uint, c_double, P]),
        "dvm_tables": (c_int, [P, P, P, c_int]),
        "dvm_text": (c_char_p, []),
        "dvm_no_arguments": (c_int, []),
    }
    assert list(got) == ["dvm_multi_line", "dvm_scalars", "dvm_tables", "dvm_text", "dvm_no_arguments"]
    for bad in ("int dvm_bad(short x);",            # a scalar parameter type without a ctypes entry
                "int dvm_bad(int a, uint64_t n);",
                "char dvm_bad(void);",              # return types
                "float *dvm_bad(int n);",
                "int dvm_bad(int (*fn)(int));",     # not a form the parser reads
                "int dvm_some_global;"):
        with pytest.raises(_lib.DvmError):
            _lib.parse_header(bad)


def test_header_entries_against_hand_written_types():
    """Five entries of the real header against types written out here by hand (the derived table is otherwise only ever compared
    with itself): long and size_t among ints, unsigned, a char * return, the longest list."""
    from ctypes import c_char_p, c_float, c_int, c_long, c_size_t, c_uint, c_void_p as P
    from dvm import _lib
    S = _lib.SIGNATURES
    bn = S["dvm_bn_act_train_fwd_pm_f32"]
    assert bn == (c_int, [P, P, P, P, c_long, c_int, c_float, c_float, c_float, P, P, P, P, P, P, c_size_t, P])
    assert len(bn[1]) == 17 and bn[1][4] is c_long and bn[1][15] is c_size_t
    assert S["dvm_linear_wgrad_f32"] == (c_int, [P, P, c_long, c_int, c_int, P, P])
    assert S["dvm_profile_select"] == (c_int, [c_uint])
    assert S["dvm_last_error"] == (c_char_p, [])
    de = S["dvm_deformer_fwd_f32"]
    assert de == (c_int, [P] * 9 + [c_int] * 6 + [P] * 10 + [P, c_int, P, c_size_t, P]) and len(de[1]) == 30


def test_loaded_prototypes_are_the_table():
    from dvm import _lib
    lib = _lib.load()
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_missing_header_is_reported(monkeypatch, tmp_path):
    from dvm import _lib
    monkeypatch.setattr(_lib, "HEADER", str(tmp_path / "include" / "dvm.h"))
    with pytest.raises(_lib.DvmError, match="dvm.h"):
        _lib._header_text()


def test_loads_and_reports_without_gpu():
    from dvm import _lib
    lib = _lib.load()
    assert lib.dvm_abi_version() == 1
    assert lib.dvm_softcorr_workspace_bytes(2, 100, 50, 128) >= (2 * 100 + 2 * 50) * 4
    assert lib.dvm_pair_direction_workspace_bytes(1, 256, 256) > 0


# (B, N, M) at d = 128 -> bytes: soft correspondence, pair, hard map one direction / both
K1_WORKSPACE_BYTES = {
    (1, 1, 1): (11264, 3116800, 8960 + 2304, 9984 + 2304),
    (2, 257, 64): (435968, 4868352, 433664 + 2304, 451840 + 2304),
    (3, 1021, 777): (3417088, 17952512, 3414784 + 2304, 3741440 + 2304),
    (2, 2048, 2048): (5099776, 25541376, 5097472 + 2304, 5671168 + 2304),
    (1, 8193, 300): (5843456, 26486272, 5841152 + 2304, 5883392 + 2304),
}


def test_k1_workspace_sizes_are_pinned():
    """The K1 workspace is one layout for the soft correspondence, the pair path and the hard map: sizes as recorded (the hard
    map's: its earlier size plus the 2304-byte block of absmax slots it now shares), and the hard map's one-direction workspace
    IS the soft correspondence's — the norms of both sides in front of the same K1 layout."""
    from dvm import _lib
    lib = _lib.load()
    for (B, N, M), (soft, pair, hard1, hard2) in K1_WORKSPACE_BYTES.items():
        got = (lib.dvm_softcorr_workspace_bytes(B, N, M, 128), lib.dvm_pair_workspace_bytes(B, N, M),
               lib.dvm_argmin_workspace_bytes(B, N, M, 128, 0), lib.dvm_argmin_workspace_bytes(B, N, M, 128, 1))
        assert got == (soft, pair, hard1, hard2), (B, N, M, got)
        assert got[2] == got[0], (B, N, M, got)


def test_no_cpu_fallback():
    import torch
    from dvm import ops
    from dvm._lib import DvmError
    f = torch.randn(1, 8, 128)
    with pytest.raises(DvmError):
        ops.softcorr(f, f, 10.0)
    with pytest.raises(DvmError):
        ops.knn_cdist(torch.rand(1, 8, 3), torch.rand(1, 8, 3), 3)


def test_linear_last_launch_before_any_launch():
    """dvm_linear_last_launch is host-only: on a thread that has launched no forward GEMM (a fresh one: the record is per thread) it
    is an argument error that names the reason and zeroes the caller's eight ints; a null pointer is refused."""
    import threading
    from ctypes import c_int, c_void_p
    from dvm import _lib
    lib = _lib.load()
    assert _lib.SIGNATURES["dvm_linear_last_launch"] == (c_int, [c_void_p])
    got = {}

    def ask():
        info = (c_int * 8)(*range(1, 9))
        got["rc"], got["msg"], got["info"] = lib.dvm_linear_last_launch(info), lib.dvm_last_error(), list(info)
        got["null"] = (lib.dvm_linear_last_launch(None), lib.dvm_last_error())

    t = threading.Thread(target=ask)
    t.start()
    t.join()
    assert got["rc"] == -1 and b"no forward GEMM launch on this thread yet" in got["msg"] and got["info"] == [0] * 8, got
    assert got["null"][0] == -1 and b"null pointer" in got["null"][1], got


def test_argument_validation_without_gpu():
    """Shape/argument errors are reported before anything touches a device."""
    from dvm import _lib
    lib = _lib.load()
    rc = lib.dvm_softcorr_fwd_f32(None, None, 1, 8, 8, 128, -1.0, 10, None, None, None, None, 0, None, 0, None)
    assert rc == -1 and b"null pointer" in lib.dvm_last_error()
    one = ctypes.c_void_p(16)
    rc = lib.dvm_softcorr_fwd_f32(one, one, 1, 8, 8, 130, -1.0, 10, one, one, None, None, 0, None, 0, None)
    assert rc == -1 and b"d=130" in lib.dvm_last_error()
    rc = lib.dvm_softcorr_fwd_f32(one, one, 1, 8, 8, 128, -1.0, 10, one, one, None, None, 0, None, 0, None)
    assert rc == -3 and b"workspace" in lib.dvm_last_error()
    rc = lib.dvm_knn_cdist_f32(one, one, 1, 8, 8, 3, 17, one, None, 0, None)
    assert rc == -1
