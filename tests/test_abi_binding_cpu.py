"""CPU-only checks of the ctypes binding: _lib derives every signature, enum value and the ABI version from
include/mpo_hip.h, and tests/golden/abi_signatures.json holds the table as it was written by hand before that (entry ->
[restype, [argtypes]] by ctypes class name, plus the enum dicts).  A header edit that changes a signature has to change
the fixture in the same commit.  The parser's refusals are checked on header text; nothing here loads the library."""
import json
import os

import pytest

from multimodal_path_omic_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _names(signatures):
    return {name: [res.__name__, [a.__name__ for a in args]] for name, (res, args) in signatures.items()}


def test_header_signatures_equal_the_recorded_table():
    with open(os.path.join(ROOT, "tests", "golden", "abi_signatures.json")) as f:
        recorded = json.load(f)
    with open(os.path.join(ROOT, "include", "mpo_hip.h")) as f:
        signatures, _, version = L.parse_header(f.read())
    derived = _names(signatures)
    assert len(recorded["signatures"]) >= 87
    assert sorted(derived) == sorted(recorded["signatures"])
    for name, want in recorded["signatures"].items():
        assert derived[name] == want, name
    assert L.exported_symbols() == list(signatures) and version == L.ABI_VERSION
    assert L.ACT == recorded["enums"]["ACT"] == {"none": 0, "relu": 1, "elu": 2, "tanh": 3, "sigmoid": 4}
    assert L.OPTIM == recorded["enums"]["OPTIM"] == {"adam": 0, "adamax": 1, "adadelta": 2, "sgd": 3}
    assert {"MPO_F32": L.MPO_F32, "MPO_BF16": L.MPO_BF16} == recorded["enums"]["DTYPE"] == {"MPO_F32": 0, "MPO_BF16": 1}


def test_parser_types_every_form_the_header_uses():
    text = """
    /* int mpo_in_a_comment(double x); */
    #define MPO_ABI_VERSION 7
    enum { MPO_ACT_NONE_ = 0, MPO_ACT_RELU_ = 1 };
    int mpo_none(void);
    const char* mpo_text(void);
    size_t mpo_size(int, int64_t n, const uint64_t*);      // unnamed parameters
    uint64_t mpo_wide(const float* const* params, const int widths[], float /* nullable */ p,
                      const mpo_bag_plan* plan, uint64_t seed, int32_t k, size_t bytes, mpo_stream_t stream);
    """
    signatures, constants, version = L.parse_header(text)
    assert _names(signatures) == {
        "mpo_none": ["c_int", []],
        "mpo_text": ["c_char_p", []],
        "mpo_size": [L.c_size_t.__name__, ["c_int", L.c_int64.__name__, "c_void_p"]],
        "mpo_wide": [L.c_uint64.__name__, ["c_void_p", "c_void_p", "c_float", "c_void_p", L.c_uint64.__name__, "c_int",
                                           L.c_size_t.__name__, "c_void_p"]],
    }
    assert constants == {"MPO_ACT_NONE_": 0, "MPO_ACT_RELU_": 1} and version == 7


def test_parser_refuses_an_unknown_scalar_type():
    for decl in ("int mpo_bad_entry(const float* x, double scale, mpo_stream_t stream);",
                 "int mpo_bad_entry(unsigned n);",
                 "double mpo_bad_entry(int n);",
                 "float* mpo_bad_entry(int n);"):
        with pytest.raises(RuntimeError, match="mpo_bad_entry") as e:
            L.parse_header("int mpo_fine(int n);\n" + decl)
        assert "no ctypes type" in str(e.value)
    with pytest.raises(RuntimeError, match="double scale"):
        L.parse_header("int mpo_bad_entry(const float* x, double scale, mpo_stream_t stream);")


def test_parser_refuses_a_declaration_that_does_not_close():
    with pytest.raises(RuntimeError, match="mpo_open_entry.*not a whole declaration"):
        L.parse_header("int mpo_open_entry(const float* x, int n;\nint mpo_fine(int n);\n")
    with pytest.raises(RuntimeError, match="mpo_open_entry"):
        L.parse_header("int mpo_fine(int n);\nint mpo_open_entry(const float* x,\n")
    with pytest.raises(RuntimeError, match="mpo_no_semicolon"):
        L.parse_header("int mpo_no_semicolon(int n)\nint mpo_fine(int n);\n")


def test_abi_version_mismatch_is_refused():
    L.check_abi_version(14, 14)
    with pytest.raises(RuntimeError, match=r"ABI version 13.*describes 14.*g\.build\(\)"):
        L.check_abi_version(13, 14)
