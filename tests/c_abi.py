"""What every ``test_new_entry_points_have_matching_argument_lists`` asserts of the entry points its file names."""
import os
import re
from ctypes import c_float, c_int, c_longlong, c_ulonglong, c_void_p

from climate2weather_amd import _lib
from climate2weather_amd import build as c2w_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"int": c_int, "long long": c_longlong, "unsigned long long": c_ulonglong, "float": c_float}


def _ctype(arg):
    arg = " ".join(arg.split())
    return c_void_p if "*" in arg else CTYPES[arg.rsplit(" ", 1)[0]]


def assert_declared(names, source=None, ops_module=None, functions=()):
    """``names``: ``{entry point: its return type in include/c2w_hip.h}``.  Every one is declared there with that return type and with
    the argument list ``_lib._PROTOS`` gives ctypes, and is among the exported symbols; ``source`` is one of the library's translation
    units; every one of ``functions`` is a launcher of ``ops_module``."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "c2w_hip.h")).read(), flags=re.S)
    for name, ret in names.items():
        m = re.search(r"([\w ]+?)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m is not None, name
        assert " ".join(m.group(1).split()) == ret, name
        assert (ret == "long long") == name.endswith("_bytes"), name  # what _lib.load() derives the return type from
        assert [_ctype(a) for a in m.group(2).split(",")] == _lib._PROTOS[name], name
    assert set(names) <= set(_lib.exported_symbols())
    if source is not None:
        assert source in c2w_build.SOURCES
    for fn in functions:
        assert callable(getattr(ops_module, fn)), fn
