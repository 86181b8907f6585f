"""tests/support/layouts.py on the CPU: every layout reads back its logical arrays bit for bit through (pointer, stride), as the library would address them;
unchanged() sees one flipped bit in a pad, in a guard band and in front of an offset base; `shared` refuses arrays whose rows differ."""
import ctypes as C

import numpy as np
import pytest

from tests.support import layouts as lo

B = 5
WIDTHS = dict(P=7, q=4, A=9, l=6, u=6)


def _arrays(seed=3):
    rng = np.random.default_rng(seed)
    a = {k: rng.standard_normal((B, w)) for k, w in WIDTHS.items()}
    a["l"][1, 2] = -np.inf; a["u"][1, 2] = np.inf; a["q"][0, 0] = -0.0          # (bit for bit: infinities and the sign of zero included)
    return a


def _through_pointer(v, batch):
    """row b read at pointer + b * stride doubles, with nothing but the two numbers the C ABI gets"""
    return np.stack([np.ctypeslib.as_array(C.cast(v.ptr + 8 * b * v.stride, C.POINTER(C.c_double)), (v.width,)).copy() for b in range(batch)])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("layout", lo.SINGLE + ("record",))
def test_every_layout_reads_back_bit_for_bit(layout):
    arrays = _arrays()
    views = lo.lay_all(arrays, layout)
    for k, v in views.items():
        assert _same_bits(_through_pointer(v, B), arrays[k]) and _same_bits(v.backing.read(k, B), arrays[k]), (layout, k)
        assert v.stride >= v.width and v.ptr % 8 == 0
    assert lo.unchanged(views)
    if layout == "record":
        assert len(lo.backings(views)) == 1 and len({v.stride for v in views.values()}) == 1 and next(iter(views.values())).stride % 2 == 1
        assert len({v.ptr % 16 for v in views.values()}) == 2          # (mixed alignments inside one record)
    else:
        lead, pad = lo._SHAPE[layout]
        for k, v in views.items():
            assert v.stride == WIDTHS[k] + pad and (v.ptr - v.backing._base) // 8 == lo.GUARD + lead


def test_what_is_not_logical_is_poison():
    for layout in lo.SINGLE + ("record",):
        for bk in lo.backings(lo.lay_all(_arrays(), layout)):
            raw = bk.buf.view(np.uint64)
            assert (raw[~bk.logical] == lo.POISON).all() and np.isnan(bk.buf[~bk.logical]).all() and not np.isnan(bk.buf[bk.logical]).any()
            assert not bk.logical[:lo.GUARD].any() and not bk.logical[-lo.GUARD:].any()          # the guard bands
    v = lo.lay(_arrays()["q"], "offset3")
    first = v.backing.fields["a"][0]
    assert first == lo.GUARD + 3 and not v.backing.logical[:first].any()


def test_shared_is_one_row_at_stride_zero_and_refuses_rows_that_differ():
    a = _arrays()["q"]
    same = np.repeat(a[:1], B, axis=0)
    v = lo.lay(same, "shared")
    assert v.stride == 0 and v.rows == 1 and _same_bits(_through_pointer(v, B), same) and _same_bits(v.backing.read("a", B), same)
    with pytest.raises(ValueError):
        lo.lay(a, "shared")
    differ = same.copy(); differ[3, 1] = -differ[3, 1]
    with pytest.raises(ValueError):
        lo.lay(differ, "shared")
    views = lo.lay_all(dict(q=same, l=_arrays()["l"]), "padded7", shared=("q",))
    assert views["q"].stride == 0 and views["l"].stride == WIDTHS["l"] + 7


def _flip(bk, at):
    bk.buf.view(np.uint64)[at] ^= np.uint64(1)


def test_unchanged_notices_one_flipped_bit():
    q = _arrays()["q"]
    v = lo.lay(q, "padded7"); bk = v.backing
    first, stride, width, _ = bk.fields["a"]
    assert bk.unchanged()
    _flip(bk, first + width)                          # the first double of the first pad
    assert not bk.unchanged()
    _flip(bk, first + width); assert bk.unchanged()
    _flip(bk, first + 2 * stride - 1)                 # the last double of the second pad
    assert not bk.unchanged()
    for at in (0, lo.GUARD - 1, -lo.GUARD, -1):       # both ends of both guard bands
        bk = lo.lay(q, "dense").backing
        _flip(bk, at)
        assert not bk.unchanged(), at
    for lead in (1, 3):
        for k in range(lead):                         # every double between the guard band and the offset base
            bk = lo.lay(q, "offset%d" % lead).backing
            _flip(bk, lo.GUARD + k)
            assert not bk.unchanged(), (lead, k)
    views = lo.lay_record(_arrays()); bk = lo.backings(views)[0]
    gap = bk.fields["q"][0] - 1                       # the double between P and q of the first record
    assert not bk.logical[gap]
    _flip(bk, gap)
    assert not lo.unchanged(views)


def test_logical_elements_may_change():
    """unchanged() is about pads and guards: the caller overwriting its own data (spoil) is not a stray write"""
    views = lo.lay_all(_arrays(), "record")
    lo.spoil(views)
    bk = lo.backings(views)[0]
    assert np.isnan(bk.buf).all() and lo.unchanged(views)


@pytest.mark.parametrize("wid", ["q20", "cp30", "q50", "cp100"])
def test_shared_vector_batches_keep_a_status_that_is_not_solved(built, wid):
    """the batches tests/test_gpu_layouts.py shares q, l or u on, checked on the CPU oracle and not discovered on the GPU: `name` is really one row, the other
    arrays still differ by instance, and the statuses are a mix of solved and not solved"""
    from optimal_control_problem_amd import models
    from tests.support import problems
    _, ls, _ = problems.hard_stage_batch(wid)
    own = lo.materialised(ls)
    for name in ("q", "l", "u"):
        a = lo.shared_vector_batch(ls, name)
        assert lo.lay(a[name], "shared").stride == 0 and not np.array_equal(a[name], own[name])
        for k in lo.FIELDS:
            if k != name:
                with pytest.raises(ValueError):
                    lo.lay(a[k], "shared")
        assert (a["l"] <= a["u"]).all()
        s = models.LocalSystem(ls.n, ls.m, ls.Pp, ls.Pi, ls.Ap, ls.Ai, a["P"], a["q"], a["A"], a["l"], a["u"], ls.np)
        status = problems.oracle_solve(s, nthreads=8)["status"]
        assert (status == 1).sum() >= ls.batch // 2 and (status != 1).any(), (wid, name, status)
