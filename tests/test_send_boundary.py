"""CPU-only: ipls_agg_send_gradients at the library's boundary -- the prototype
in include/ipls_agg.h, the exported symbol, the ctypes binding, the new kernel
ID, and an ABI version that stays 4 because the call is additive."""
import ctypes
import fnmatch
import re

from conftest import ROOT

NAME = "ipls_agg_send_gradients"
PARAMS = ["ipls_agg *h", "const void *flat", "int64_t n", "int src_kind", "const int32_t *parts", "int n_parts",
          "int32_t iteration", "int16_t pid", "const uint8_t *origin", "int32_t origin_len", "void *out",
          "int64_t out_cap", "int out_kind", "int64_t *lens", "int64_t *offs"]


def header():
    return (ROOT / "include" / "ipls_agg.h").read_text()


def test_prototype_is_in_the_header():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"int64_t\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{NAME} is not declared"
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == PARAMS


def test_header_comment_states_the_contract():
    text = header()
    doc = text[text.index("send-side codec"):text.index("int64_t " + NAME)]
    for phrase in ("-0.0", "count slot", "ONE base64 layer", "Middleware.Encode is not applied", "ipls_agg_split",
                   "flat == NULL", "IPLS_E_RANGE"):
        assert phrase in doc, phrase


def test_symbol_is_exported():
    """exports.map makes the C-ABI's names global and nothing else; the built library carries the new one."""
    text = (ROOT / "ipls-java-api_amd" / "csrc" / "exports.map").read_text()
    globs = re.search(r"global:\s*([^;]+);", text).group(1).split()
    assert any(fnmatch.fnmatchcase(NAME, g) for g in globs)
    import ipls
    assert hasattr(ipls.lib(), NAME), f"{NAME} is not exported by the library"


def test_binding_has_the_signature():
    from ipls import _native as N
    assert NAME in N.SIGNATURES
    res, args = N.SIGNATURES[NAME]
    assert res is ctypes.c_int64 and len(args) == len(PARAMS)
    scalars = {2: ctypes.c_int64, 3: ctypes.c_int, 5: ctypes.c_int, 6: ctypes.c_int32, 7: ctypes.c_int16,
               9: ctypes.c_int32, 11: ctypes.c_int64, 12: ctypes.c_int}
    for i, a in enumerate(args):
        assert a is scalars.get(i, ctypes.c_void_p), (i, PARAMS[i], a)
    rc = getattr(N.lib(), NAME)(None, None, 0, N.HOST_F64, None, 0, 0, 3, None, 0, None, 0, N.HOST_TEXT, None, None)
    assert rc == N.IPLS_E_INVAL and "null" in N.last_error(None)


def test_kernel_id_and_abi():
    import ipls
    from ipls import _native as N
    defs = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define\s+(IPLS_\w+)\s+\(?(-?\d+)\)?", header()))
    assert defs["IPLS_KERNEL_ENCODE_FLAT"] == 12 == N.KERNEL_ENCODE_FLAT == ipls.KERNEL_ENCODE_FLAT
    kernels = sorted(v for k, v in defs.items() if k.startswith("IPLS_KERNEL_"))
    assert kernels == list(range(1, 13))                       # additive: the earlier IDs keep their values
    assert defs["IPLS_AGG_ABI_VERSION"] == 4 == N.ABI_VERSION == N.lib().ipls_agg_abi_version()
    assert ctypes.sizeof(N.LaunchInfo) == 48


def test_python_front_takes_the_call():
    import inspect

    import ipls
    sig = inspect.signature(ipls.Aggregator.SendGradients)
    assert list(sig.parameters)[:4] == ["self", "gradients", "partitions", "iteration"]
    for name, default in (("origin", b""), ("pid", 3), ("out", None)):
        p = sig.parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == default
