"""CPU-only: host.PROTOTYPES, the ctypes mirror of csrc/host/srt_host_c.h, against the header itself (argument by argument, with the
parser and the check test_abi_mirror.py uses for include/srt.h), the header against what libsrt_host.so exports and against a C
compiler, and doctored headers and tables to show that the check can fail."""
import ctypes as C
import os
import re
import subprocess

import pytest

from header_mirror import check_prototypes, expected_argtype, parse_header
from simple_raytracer_amd import abi, build, host

HEADER = os.path.join(build.HOST_DIR, "srt_host_c.h")


def host_argtype(function, c_type, parameter, structs):
    """The rule of host.py: a string, in or out, is c_char_p; every handle is void*; the rest as for include/srt.h."""
    return C.c_char_p if c_type == "char*" else expected_argtype(function, c_type, parameter, structs)


def check(table, text):
    return check_prototypes(table, abi.STRUCTS, parse_header(text, prefix="srth_"), argtype=host_argtype)


@pytest.fixture(scope="module")
def text():
    return open(HEADER).read()


def test_table_matches_the_header(text):
    declared = [name for name, _, _ in parse_header(text, prefix="srth_")["prototypes"]]
    assert len(declared) == 51 and len(set(declared)) == 51
    assert check(host.PROTOTYPES, text) == []
    assert list(host.PROTOTYPES) == declared, "the table follows the header's order"
    for name, (restype, argtypes) in host.PROTOTYPES.items():      # what ctypes accepts: a list of types, a type or None
        assert isinstance(argtypes, list) and (restype is None or isinstance(restype, type(C.c_int))), name


def test_every_exported_function_is_declared(text):
    build.build_all()
    out = subprocess.run(["nm", "-D", "--defined-only", host.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(srth_\w+)$", out, flags=re.M))
    assert exported == set(host.PROTOTYPES), exported ^ set(host.PROTOTYPES)
    L = host.load()
    for name, (restype, argtypes) in host.PROTOTYPES.items():      # and load() has given every one its types
        assert getattr(L, name).restype is restype and getattr(L, name).argtypes == argtypes, name


def test_header_is_plain_c(tmp_path):
    (tmp_path / "only.c").write_text(f'#include "{HEADER}"\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", str(tmp_path / "only.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_check_can_fail(text):
    """A doctored copy of the header, a doctored table: each fault is reported, and by the function's name."""
    def only(errors, name):
        assert errors and all(e.startswith(name + ":") for e in errors), errors
        return errors

    wide = text.replace("int srth_om_add_texture(void* om, const char* texname, int32_t w,", "int srth_om_add_texture(void* om, const char* texname, int64_t w,")
    assert wide != text and "argument 2 (int64_t w)" in only(check(host.PROTOTYPES, wide), "srth_om_add_texture")[0]
    gone = text.replace("void srth_multi_free(void* r);", "")
    assert gone != text and "in the table, not in the header" in only(check(host.PROTOTYPES, gone), "srth_multi_free")[0]
    other_return = text.replace("int64_t srth_om_num_tris(", "int srth_om_num_tris(")
    assert other_return != text and "restype" in only(check(host.PROTOTYPES, other_return), "srth_om_num_tris")[0]

    def doctored(name, change):
        table = dict(host.PROTOTYPES)
        restype, argtypes = table[name]
        table[name] = change(restype, list(argtypes))
        return only(check(table, text), name)
    doctored("srth_renderer_render_posed", lambda r, a: (r, a[:6] + [C.c_int] + a[7:]))     # n_mats as int
    doctored("srth_flat_names", lambda r, a: (r, [a[0], C.POINTER(C.c_char), a[2]]))
    doctored("srth_multi_new", lambda r, a: (C.c_int, a))                                    # a handle cut to 32 bits
    doctored("srth_renderer_fast_frames", lambda r, a: (C.c_uint32, a))
    assert "argtypes for" in doctored("srth_render", lambda r, a: (r, a[:-1]))[0]
    missing = {k: v for k, v in host.PROTOTYPES.items() if k != "srth_renderer_collect"}
    assert "in the header, not in the table" in only(check(missing, text), "srth_renderer_collect")[0]
    only(check({**host.PROTOTYPES, "srth_extra": (None, [])}, text), "srth_extra")
