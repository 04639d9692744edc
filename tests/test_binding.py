"""CPU: the ctypes binding is declared from include/sehip.h -- the header parser, the constants it exposes, and the checks of
``_lib.call`` against stub entry points (no library function and no GPU is involved)."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def stub(monkeypatch):
    """Replace the loaded library by stub entry points that record their arguments; the stream is a sentinel."""
    from sehip import _lib
    calls = []
    stream = ctypes.c_void_p(0x5E)

    def entry(name, rc):
        def fn(*args):
            calls.append((name, args))
            return rc
        return fn
    names = {"se_relevant_positions": 0, "se_relevant_positions_r16": 0, "se_hprec_curve_len": 4096 + 7, "se_row_sqnorm": 0,
             "se_phase_timing": -1, "se_last_error": b"stub failure"}
    monkeypatch.setattr(_lib, "_lib", types.SimpleNamespace(**{n: entry(n, rc) for n, rc in names.items()}))
    monkeypatch.setattr(_lib, "stream_ptr", lambda: stream)
    return _lib, calls, stream


def _relevant_positions_args(rank):
    i32 = torch.zeros(4, dtype=torch.int32)
    return (rank, 4, 2, 4, i32, 4, i32, None, 3, torch.zeros(3, dtype=torch.int64), i32)


def test_parse_header_reads_prototypes_and_defines():
    from sehip._lib import SehipError, parse_header
    protos, defines = parse_header("""
        #define SE_A 3
        #define SE_B (-2)   /* negative, parenthesised */
        #define SE_NAME_ONLY
        // int se_commented(double x);
        /* int se_also_commented(size_t n); */
        typedef void *se_stream_t;
        int64_t se_size(void);
        const char *se_text(void);
        int se_k(const uint16_t *rank, int64_t n, float s, uint32_t *mask, const char **names_host,
                 se_stream_t stream);
        int se_host(int on);
    """)
    assert defines == {"SE_A": 3, "SE_B": -2}
    assert sorted(protos) == ["se_host", "se_k", "se_size", "se_text"]
    assert protos["se_size"].restype == "int64_t" and protos["se_size"].params == () and not protos["se_size"].stream
    assert protos["se_text"].restype == "const char *"
    k = protos["se_k"]
    assert k.restype == "int" and k.stream
    assert [(p.ctype, p.pointee, p.name) for p in k.params] == [
        ("uint16_t *", "uint16_t", "rank"), ("int64_t", None, "n"), ("float", None, "s"), ("uint32_t *", "uint32_t", "mask"),
        ("char * *", "char *", "names_host")]
    assert [p.ctype for p in protos["se_host"].params] == ["int"] and not protos["se_host"].stream
    with pytest.raises(SehipError, match="se_cb"):
        parse_header("int se_cb(int (*fn)(int));")          # a declaration the parser cannot read is an error, not skipped


@pytest.mark.parametrize("decl", ["int se_bad(const float *x, size_t n, se_stream_t stream);",
                                  "int se_bad(double scale);",
                                  "int se_bad(const uint8_t *bytes);",
                                  "int se_bad(unsigned int n);",
                                  "double se_bad(int n);"])
def test_parse_header_rejects_unknown_types_and_names_the_declaration(decl):
    from sehip._lib import SehipError, parse_header
    with pytest.raises(SehipError, match="se_bad"):
        parse_header("int se_fine(int n);\n" + decl)


def test_every_exposed_constant_equals_its_define():
    import sehip
    from sehip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sehip.h")).read(), flags=re.S)
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(SE_\w+)\s+\(?(-?\d+)\)?", src)}
    exposed = {"SE_OK": "SE_OK", "DTYPE_F32": "SE_DTYPE_F32", "DTYPE_BF16": "SE_DTYPE_BF16", "METRIC_COSINE": "SE_METRIC_COSINE",
               "METRIC_EUCLID": "SE_METRIC_EUCLID", "METRIC_DOT": "SE_METRIC_DOT", "SVM_GRAD": "SE_SVM_GRAD", "SVM_HV": "SE_SVM_HV",
               "SVM_SCORE": "SE_SVM_SCORE", "TOPK_MAX": "SE_TOPK_MAX"}
    for py, c in exposed.items():
        assert getattr(_lib, py) == defines[c], py
        if py != "SE_OK":
            assert getattr(sehip, py) == defines[c], py
    assert _lib.DEFINES == defines


def test_loader_declares_the_parsed_signatures():
    """What a slip of the hand-written table would have broken: int vs int64_t scalars shift every later argument."""
    import sehip
    L = sehip.lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert L.se_topk_rows.argtypes == [vp, i64, i64, i64, i64, i32, vp, vp, vp]
    assert L.se_topk_rows.restype is i32
    assert L.se_svm_margin.argtypes[10] is ctypes.c_float
    assert L.se_retrieve_topk_workspace_bytes.restype is i64
    assert L.se_last_error.restype is ctypes.c_char_p and L.se_last_error.argtypes == []
    for name, proto in sehip._lib.PROTOTYPES.items():
        assert len(getattr(L, name).argtypes) == len(proto.params) + proto.stream, name


def test_call_rejects_a_wrong_dtype_for_a_typed_pointer(stub):
    _lib, calls, _ = stub
    args = list(_relevant_positions_args(torch.zeros((2, 4), dtype=torch.int32)))
    args[4] = torch.zeros(4, dtype=torch.int64)       # const int32_t *cls
    with pytest.raises(_lib.SehipError, match="cls"):
        _lib.call("se_relevant_positions", *args)
    with pytest.raises(_lib.SehipError):              # int16 ranks are uint16_t patterns: not the int32_t entry point's
        _lib.call("se_relevant_positions", *_relevant_positions_args(torch.zeros((2, 4), dtype=torch.int16)))
    with pytest.raises(_lib.SehipError):              # one argument short
        _lib.call("se_relevant_positions", *_relevant_positions_args(torch.zeros((2, 4), dtype=torch.int32))[:-1])
    assert calls == []


def test_call_accepts_int16_for_uint16_and_passes_data_pointers(stub):
    _lib, calls, stream = stub
    for dtype in (torch.int16, torch.uint16):
        rank = torch.zeros((2, 4), dtype=dtype)
        args = _relevant_positions_args(rank)
        assert _lib.call("se_relevant_positions_r16", *args) == 0
        name, got = calls.pop()
        assert name == "se_relevant_positions_r16" and len(got) == 12 and got[-1] is stream
        assert got[0] == rank.data_ptr() and got[9] == args[9].data_ptr()               # addresses, for the declared c_void_p
        assert got[1:4] == (4, 2, 4) and got[7] is None and got[8] == 3                # everything else passes unchanged


def test_call_turns_none_into_null(monkeypatch):
    """Through the real library: its host-side argument checks run before any device work and see the NULL."""
    from sehip import _lib
    _lib.lib()
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    with pytest.raises(_lib.SehipError, match="se_pairwise_dist failed .*null pointer"):
        _lib.call("se_pairwise_dist", None, 4, None, 4, None, None, 2, 2, 4, 0, None, 0, None, 2)


def test_call_appends_the_stream_only_when_the_prototype_ends_in_one(stub):
    _lib, calls, stream = stub
    x = torch.zeros((3, 5), dtype=torch.float32)
    _lib.call("se_row_sqnorm", x, 5, 3, 5, torch.zeros(3))
    assert calls.pop()[1][-1] is stream
    assert _lib.call("se_hprec_curve_len", 4096) == 4096 + 7                           # an int64_t size query returns its value
    assert calls.pop()[1] == (4096,)


def test_call_raises_on_a_negative_status(stub):
    _lib, calls, _ = stub
    with pytest.raises(_lib.SehipError, match="se_phase_timing failed .*stub failure"):
        _lib.call("se_phase_timing", 1)
