"""CPU tier for the editing calls (include/gs_splat.h: gs_set_state ... gs_compact): the built library exports them, and the constants
of the ctypes binding are those of the header."""
import ctypes as C
import os
import re

from conftest import ROOT, pkg

capi = pkg("capi")

NEW = ["gs_set_state", "gs_set_state_ids", "gs_state_count", "gs_select_box", "gs_select_sphere", "gs_select_rect", "gs_compact",
       "gs_multi_set_state", "gs_multi_set_state_ids", "gs_multi_select_box", "gs_multi_select_sphere", "gs_multi_select_rect",
       "gs_multi_compact"]


def _header():
    with open(os.path.join(ROOT, "include", "gs_splat.h")) as f:
        return f.read()


def _define(name):
    m = re.search(r"^#define\s+%s\s+(\d+)u?\b" % name, _header(), re.M)
    assert m, name
    return int(m.group(1))


def test_symbols_are_declared_exported_and_bound():
    hdr = _header()
    L = capi.load()
    for name in NEW:
        assert re.search(r"GS_API\s+int\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in capi.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name


def test_constants_agree_with_the_header():
    assert capi.STATE_HIDDEN == _define("GS_STATE_HIDDEN") == 1
    assert capi.STATE_SELECTED == _define("GS_STATE_SELECTED") == 2
    assert capi.SELECT_INVERT == _define("GS_SELECT_INVERT") == 1
    assert capi.BUF_STATE == _define("GS_BUF_STATE") == 9


def test_stats_carry_n_hidden_where_the_header_puts_it():
    names = [n for n, _ in capi.Stats._fields_]
    fields = re.search(r"typedef struct gs_stats \{(.*?)\} gs_stats;", _header(), re.S).group(1)
    declared = re.findall(r"\b(\w+)\s*(?:,|;)", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert "n_hidden" in names and names == declared
    assert dict(capi.Stats._fields_)["n_hidden"] is C.c_uint32 and names[-5:] == ["n_hidden", "surface", "antialias", "seg_count", "n_runs"]


def test_null_context_is_refused_without_a_gpu():
    L = capi.load()
    assert L.gs_set_state(None, 0, None, 0) == capi.E_BADARG
    assert L.gs_set_state_ids(None, None, 0, 0, 0) == capi.E_BADARG
    assert L.gs_state_count(None, None, None) == capi.E_BADARG
    assert L.gs_select_box(None, None, 0, 0, 0, None) == capi.E_BADARG
    assert L.gs_select_sphere(None, None, 0.0, 0, 0, 0, None) == capi.E_BADARG
    assert L.gs_select_rect(None, None, None, 0, 0, 0, None) == capi.E_BADARG
    assert L.gs_compact(None, None, None) == capi.E_BADARG
    assert L.gs_multi_compact(None, None, None) == capi.E_BADARG
