"""GPU tier of gs_set_option (include/gs_splat.h): every option's accepted range, its message when a value lies outside, the unknown option.

A context with no splats: every case is a host call.  The messages are the library's, byte for byte: a caller that shows gs_last_error to
its user sees these strings.  An option without a bound on one side (or on both: a switch that reads `value != 0`) has no value to
refuse there; the int64 extreme is its edge."""
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu
capi = pkg("capi")

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
U32_MAX = 0xFFFFFFFF

# (option, lowest accepted value or None, highest accepted value or None, the message for a value outside)
RANGES = [
    (capi.OPT_PROFILE, None, None, None),
    (capi.OPT_TERMINATION, 2, None, "termination 1/eps must be >= 2"),
    (capi.OPT_NEAR_PERMILLE, 0, 1000, "near permille must be 0 (adaptive) .. 1000 (single round)"),
    (capi.OPT_RECORD_STAGED, None, None, None),
    (capi.OPT_PIPELINE_DEPTH, 1, 4, "pipeline depth must be 1..4"),
    (capi.OPT_WIDE_PAIRS, 0, 1, "wide records: 0 (automatic) or 1 (the depth sort's general 8-byte records whatever the number of splats)"),
    (capi.OPT_ENQUEUE_THREADS, None, None, None),
    (capi.OPT_COMM_SELF_COPY, None, None, None),
    (capi.OPT_BLEND_SPLIT, 0, 0x7FFFFFFF, "blend split: 0 (off) or the list length from which a tile is split"),
    (capi.OPT_FRAME_BATCH, 1, 2, "frame batch must be 1 (off) or 2"),
    (capi.OPT_SORT_NEAR, 0, 2, "near-only sorts: 0 (off), 1 (scenes of 4 M splats and more) or 2 (always)"),
    (capi.OPT_COMM_TRANSPORT, 0, 1, "comm transport: 0 (RCCL) or 1 (in-process)"),
    (capi.OPT_AUTO_RETRY, None, None, None),
    (capi.OPT_SORT_SHARE, 0, 1000, "sort share: 0 (off) or the permille of the splats whose order the ranks exchange"),
    (capi.OPT_BINNING, 0, 1, "binning: 0 (span lists wherever the strip fits) or 1 (pair records and two stable radix passes)"),
    (capi.OPT_SUBTILE, 0, 2, "sub-tile lists: 0 (off), 1 (where splats are small) or 2 (always)"),
    (capi.OPT_ROW_WALK, 0, 2, "row walk: 0 (off), 1 (where splats are large) or 2 (always)"),
    (capi.OPT_SH_DEGREE, 0, 3, "spherical-harmonics degree: 0 (off) to 3"),
    (capi.OPT_ANTIALIAS, 0, 1, "anti-aliased splats: 0 (off) or 1 (opacity compensated for the 0.3 px^2 dilation)"),
    (capi.OPT_SEG_COUNT, 0, 2, "segment counts: 0 (never), 1 (where tile rows hold many runs) or 2 (always)"),
    (capi.OPT_SORT_NEAR_FORCE, 0, U32_MAX, "forced near-only sorts: 0 (the policy decides) or the positions every sort without an index list is asked for"),
    (capi.OPT_HIGHLIGHT, 0, U32_MAX, "highlight: R | G << 8 | B << 16 | W << 24 (W = 0: off)"),
]
IDS = {v: k for k, v in vars(capi).items() if k.startswith("OPT_")}


def test_every_option_of_the_header_is_listed():
    """the table above against include/gs_splat.h: no option without a row"""
    import os
    import re
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gs_splat.h")
    with open(header) as f:
        declared = {int(m.group(1)) for m in re.finditer(r"^#define GS_OPT_\w+\s+(\d+)", f.read(), re.M)}
    assert declared == {r[0] for r in RANGES}


def set_option(ctx, opt, value):
    """(return code, gs_last_error) of one call"""
    rc = ctx._L.gs_set_option(ctx._h, int(opt), int(value))
    return rc, ctx._L.gs_last_error(ctx._h).decode()


@pytest.fixture(scope="module")
def ctx():
    with capi.Context(0) as c:
        yield c


@pytest.mark.parametrize("opt,lo,hi,msg", RANGES, ids=[IDS[r[0]] for r in RANGES])
def test_range_and_message(ctx, opt, lo, hi, msg):
    # outside first, then the edges: the option is left at an accepted value
    if lo is not None:
        assert set_option(ctx, opt, lo - 1) == (capi.E_BADARG, msg)
        assert set_option(ctx, opt, I64_MIN) == (capi.E_BADARG, msg)
    if hi is not None:
        assert set_option(ctx, opt, hi + 1) == (capi.E_BADARG, msg)
        assert set_option(ctx, opt, I64_MAX) == (capi.E_BADARG, msg)
    for edge in (I64_MIN if lo is None else lo, I64_MAX if hi is None else hi):
        assert set_option(ctx, opt, edge)[0] == capi.GS_OK, (IDS[opt], edge)
    if lo is None and hi is None:                                # a switch: 0 and the profile's three modes too
        for v in (3, 2, 1, 0):
            assert set_option(ctx, opt, v)[0] == capi.GS_OK, (IDS[opt], v)


def test_a_refused_value_changes_nothing(ctx):
    """the range is checked before the store (the one option whose value can be read back: gs_highlight_info)"""
    assert set_option(ctx, capi.OPT_HIGHLIGHT, 0x11223344)[0] == capi.GS_OK
    assert set_option(ctx, capi.OPT_HIGHLIGHT, U32_MAX + 1)[0] == capi.E_BADARG
    assert ctx.highlight_info()[0] == 0x11223344
    assert set_option(ctx, capi.OPT_HIGHLIGHT, 0)[0] == capi.GS_OK


@pytest.mark.parametrize("opt", [0, 14, 24, -1, 1 << 20])
def test_unknown_option(ctx, opt):
    assert set_option(ctx, opt, 1) == (capi.E_BADARG, "unknown option %d" % opt)
