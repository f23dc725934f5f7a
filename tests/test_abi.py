"""CPU: the C-ABI library loads and exports every symbol include/mdm_hip.h declares (no compute without a GPU)."""
import ctypes as C
import os
import re

from conftest import ROOT, pkg


def _header():
    """include/mdm_hip.h without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdm_hip.h")).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(mdm_[a-z0-9_]+)\s*\(", _header())))


def test_library_exports_every_declared_symbol():
    L = pkg("_lib")
    if not os.path.exists(L.LIB_PATH):
        pkg("build").build(verbose=False)
    lib = L.lib()
    names = _declared()
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mdm_hip.h but not exported"
    assert set(L.EXPORTS) == set(names), (set(L.EXPORTS) ^ set(names))
    assert lib.mdm_version().startswith(b"mdm_hip")


_CTYPE = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
          "double": C.c_double}


def _ctype(decl):
    """The ctypes type of one C parameter or return type: every pointer is c_void_p (``const char*`` returned: c_char_p)."""
    if "*" in decl:
        return C.c_void_p
    return _CTYPE[decl.replace("const", "").strip()]


def _header_prototypes():
    """name -> (restype, [argtypes]) of every function include/mdm_hip.h declares."""
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?[\s*]+)(mdm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header()):
        params = [p.strip() for p in params.split(",") if p.strip() not in ("", "void")]
        args = [_ctype(re.match(r"(.*?)\w+$", p, flags=re.S).group(1)) for p in params]  # drop the parameter's name
        protos[name] = (C.c_char_p if "char" in ret else _ctype(ret), args)
    return protos


def test_prototypes_match_the_header():
    """_lib.PROTOTYPES states every declaration of the header: the same names, arity and types, position by position."""
    L = pkg("_lib")
    want = _header_prototypes()
    assert sorted(want) == _declared() and len(want) >= 70
    assert set(L.PROTOTYPES) == set(want), set(L.PROTOTYPES) ^ set(want)
    assert L.EXPORTS == list(L.PROTOTYPES)
    for name, (restype, argtypes) in want.items():
        ours = L.PROTOTYPES[name]
        assert len(ours[1]) == len(argtypes), name
        assert ours == (restype, argtypes), (name, ours, (restype, argtypes))
    assert want["mdm_version"] == (C.c_char_p, [])
    lib = L.lib()
    for name, (restype, argtypes) in L.PROTOTYPES.items():  # and lib() has put them on the loaded symbols
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_struct_mirrors_match_c_layout(tmp_path):
    """ctypes mirrors in _lib.py must agree with the C structs (compiled with g++ on the fly): sizeof and the offsetof of every
    field, the field list taken from each mirror's _fields_ (the C name is the Python one, but global_ -> global)."""
    import subprocess
    L = pkg("_lib")
    mirrors = {"MdmOperand": L.Operand, "MdmGemmDesc": L.GemmDesc, "MdmMlpDesc": L.MlpDesc, "MdmPacked": L.Packed,
               "MdmStyle": L.Style, "MdmPerformer": L.Performer, "MdmLayer": L.Layer, "MdmModel": L.Model,
               "MdmTextCache": L.TextCache, "MdmStemCache": L.StemCache, "MdmSkeleton": L.Skeleton, "MdmMoeTensors": L.MoeTensors}
    assert set(mirrors) == set(re.findall(r"\}\s*(Mdm\w+)\s*;", _header())), "a struct of the header has no mirror here"
    lines, ours = [], []
    for cname, mirror in mirrors.items():
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        ours.append(C.sizeof(mirror))
        for field in mirror._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {"global" if field[0] == "global_" else field[0]}));')
            ours.append(getattr(mirror, field[0]).offset)
    src = tmp_path / "sz.cpp"
    src.write_text('#include "mdm_hip.h"\n#include <cstddef>\n#include <cstdio>\nint main(){\n' + "\n".join(lines) + "\n}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    theirs = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert len(theirs) == len(ours)
    for what, a, b in zip(lines, theirs, ours):
        assert a == b, (what, a, b)
    assert theirs == ours


def test_mismatched_call_is_refused_before_the_call():
    """The failure the prototypes exist to catch, on the loaded library and without a GPU: a c_int32 instance for an int64_t
    parameter raises ctypes.ArgumentError, and one argument too few is refused by ctypes as well (CPython reports a count below
    the prototype's as TypeError, not ArgumentError).  With the header's types the same calls reach the library's own checks."""
    import pytest
    L = pkg("_lib")
    lib = L.lib()
    assert lib.mdm_route_dump(None, 0) == 0
    with pytest.raises(C.ArgumentError):
        lib.mdm_route_dump(None, C.c_int32(0))
    with pytest.raises(TypeError, match="takes at least 2 arguments"):
        lib.mdm_route_dump(None)
    assert lib.mdm_fill_timesteps_mapped(None, 0, None, None, 0, None) == 1  # MDM_ERR_ARG
    with pytest.raises(C.ArgumentError):
        lib.mdm_fill_timesteps_mapped(None, C.c_int32(0), None, None, 0, None)
    with pytest.raises(TypeError, match="takes at least 6 arguments"):
        lib.mdm_fill_timesteps_mapped(None, 0, None, None, 0)


def test_argument_validation_without_gpu():
    """Entry points reject bad descriptors before touching the device."""
    L = pkg("_lib")
    lib = L.lib()
    assert lib.mdm_gemm(None, None) == 1
    d = L.GemmDesc()
    d.M = d.N = d.K = 8
    d.batch = d.nb2 = 1
    assert lib.mdm_gemm(C.byref(d), None) == 1  # null operands
    assert lib.mdm_workspace_bytes(None, 1, 2, 1) == -1
    assert lib.mdm_cfg_posterior_step(None, None, None, None, C.c_int64(0), None, 0, None, 0, C.c_float(1.0), 0, None, None, None) == 1


def _variants():
    """The values of enum MdmVariant in include/mdm_hip.h."""
    src = open(os.path.join(ROOT, "include", "mdm_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"enum MdmVariant \{(.*?)\};", src, flags=re.S).group(1), flags=re.S)
    return {int(v) for v in re.findall(r"MDM_VAR_\w+\s*=\s*(\d+)", body)}


def test_gemm_variant_accepts_exactly_the_enum():
    """mdm_set_gemm_variant accepts the values of enum MdmVariant (the reference paths the tests hold other paths against) and
    returns MDM_ERR_ARG for every other value.  The library has no diagnostic entry points, and its fused-MLP object holds only the
    plain (0) and the Performer-tail (1) instantiations."""
    import subprocess
    L = pkg("_lib")
    lib = L.lib()
    known = _variants()
    assert known == {0, 6, 22, 23, 24, 26, 27, 34, 35, 36, 50, 51, 52, 56, 60, 61, 62, 63, 68, 69, 70}
    for v in range(1, 128):
        assert lib.mdm_set_gemm_variant(v) == (0 if v in known else 1), v  # MDM_OK / MDM_ERR_ARG
    assert lib.mdm_set_gemm_variant(0) == 0
    for name in ("mdm_diag_build", "mdm_diag_mlp_counters", "mdm_debug_stamps"):
        assert not hasattr(lib, name), name
    # template arguments <format, RT, NJ, DIN, TAIL>
    obj = os.path.join(ROOT, "motiondiffusion-moe_amd", "csrc", "build", "mlp_stream.o")
    if os.path.exists(obj):
        syms = subprocess.run(["nm", "-C", obj], capture_output=True, text=True).stdout
        tails = set(re.findall(r"fused_mlp_stream_kernel<[^,]+, \d+, \d+, \d+, (\d+)>", syms))
        assert tails == {"0", "1"}, tails
