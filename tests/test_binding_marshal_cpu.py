"""CPU: what the twelve fused-step methods of physicl_amd._hip (eight of ``Device``, four of ``DeviceGroup``) put over
the C ABI and what they hand back, on a stand-in for the library (no GPU, no libphysicl_hip.so).

The stand-in records every ``pcl_*`` call -- numbers as Python values, ``bytes`` as they are, pointers resolved to the
contents they point at (it knows each entry point's argument list), ``None`` as ``None``, the output buffer as "OUT" --
and fills the output buffer with 100, 101, 102, ...  Calls and answers are compared with their types (``int`` is not
``np.int64``, a list is not an array, dict keys in order).  Every expectation is written out below."""
import ctypes

import numpy as np
import pytest

from physicl_amd import _hip

I8, F8, I4 = np.int64, np.float64, np.int32


def _rows(k, n_planes):
    return k * (5 + max(n_planes, 0))


# entry point -> (index of every input array: (dtype, elements)), (index of the output buffer, dtype, elements)
_ABI = {
    "pcl_step_fused": lambda a: ({12: (F8, 3 * max(a[13], 0))}, (14, I8, 5 + a[13])),
    "pcl_step_fused_multi": lambda a: ({11: (F8, 3 * a[12])}, (13, I8, _rows(a[2], a[12]))),
    "pcl_step_mixed_multi": lambda a: ({4: (I4, a[3]), 15: (F8, 3 * a[16])}, (17, I8, _rows(a[2] * a[3], a[16]))),
    "pcl_store_trace_ahead": lambda a: ({1: (I8, a[2]), 6: (I4, a[5])}, (18, F8, a[4] * a[2] * 4)),
    "pcl_store_trace_read": lambda a: ({}, (1, F8, a[2])),
    "pcl_step_fused_read": lambda a: ({}, (2, I8, 5 + a[1])),
    "pcl_step_fused_delete": lambda a: ({8: (F8, 3 * max(a[9], 0))}, (10, I8, _rows(1, a[9]))),
    "pcl_step_fused_delete_multi": lambda a: ({7: (F8, 3 * max(a[8], 0))}, (9, I8, _rows(a[2], a[8]))),
    "pcl_step_counters": lambda a: ({1: (F8, 3 * a[2])}, (3, I8, 4 + a[2])),
}
for _name in ("step_fused_multi", "step_fused_delete", "step_fused_delete_multi", "step_mixed_multi"):
    _ABI["pcl_group_" + _name] = _ABI["pcl_" + _name]


def _at(pointer, dtype, count):
    """The ``count`` elements behind ``pointer`` (a c_void_p or a plain address) as a numpy view."""
    addr = pointer.value if isinstance(pointer, ctypes.c_void_p) else pointer
    if count == 0:
        return np.zeros(0, dtype=dtype)
    assert isinstance(addr, int) and addr != 0, pointer
    return np.ctypeslib.as_array((np.ctypeslib.as_ctypes_type(dtype) * count).from_address(addr))


class FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        spec = _ABI[name]

        def call(*args):
            args = list(args)
            inputs, (out_at, out_dtype, out_count) = spec(args)
            for at, (dtype, count) in inputs.items():
                if args[at] is not None:
                    args[at] = _at(args[at], dtype, count).tolist()
            if args[out_at] is not None:
                _at(args[out_at], out_dtype, out_count)[:] = 100 + np.arange(out_count)
                args[out_at] = "OUT"
            self.calls.append((name, tuple(args)))
            return 0
        return call


def same(a, b):
    if type(a) is not type(b):
        return False
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return a == b


def cnt(N, sign, planes, phase=None, **event):
    """The dict form of one counter row, as the methods return it."""
    d = {} if phase is None else {"phase": phase}
    d.update(N=N, sign=np.array(sign, dtype=I8), planes=np.array(planes, dtype=I8))
    d.update(event)
    return d


def arrays(x):
    if isinstance(x, dict):
        return [v for v in x.values() if isinstance(v, np.ndarray)]
    return [a for d in x for a in arrays(d)]


def owned(x):
    """Every array of the answer is its own copy: no view of a shared buffer."""
    return all(a.base is None for a in arrays(x))


@pytest.fixture
def dev():
    d = _hip.Device.__new__(_hip.Device)
    d.lib, d.ctx, d.device = FakeLib(), None, 0      # (ctx None: __del__ has nothing to destroy)
    return d


@pytest.fixture
def grp():
    g = _hip.DeviceGroup.__new__(_hip.DeviceGroup)
    g.lib, g.g, g.n = FakeLib(), None, 2
    return g


def check(obj, got, call, want):
    assert len(obj.lib.calls) == 1
    assert same(obj.lib.calls[0], call), (obj.lib.calls[0], call)
    assert same(got, want), (got, want)
    obj.lib.calls.clear()


ROWS = [[1, 2, 3], [4, 5, 6]]                       # two planes
FLAT = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
READY = np.array(ROWS, dtype=np.float64)
FORTRAN = np.asfortranarray(READY)
FULL = dict(A=1, n=2.5, flags=3, c=4, h=5.5, n_expr="r0[gid]", rng_mode=0, seed=9, step=2 ** 32 + 7)
BIG = 3 * 2 ** 32 + 11                              # a launch index above 2^32: its low word is 11


def test_fortran_fixture_is_not_c_contiguous():
    assert not FORTRAN.flags.c_contiguous and READY.flags.c_contiguous


# ------------------------------------------------------------------------------------------------ Device.step_fused
def test_step_fused(dev):
    check(dev, dev.step_fused(2),
          ("pcl_step_fused", (None, 2.0, 0, 0.0, 0.0, 0, 0.0, 0.0, None, 1, 0, 0, None, -1, None)), None)
    check(dev, dev.step_fused(0.5, {}, ()),
          ("pcl_step_fused", (None, 0.5, 0, 0.0, 0.0, 0, 0.0, 0.0, None, 1, 0, 0, None, 0, "OUT")),
          cnt(100, [101, 102, 103], [], hits=104))
    got = dev.step_fused(0.5, FULL, (), lazy=True)
    assert owned(got)
    check(dev, got,
          ("pcl_step_fused", (None, 0.5, 1, 1.0, 2.5, 7, 4.0, 5.5, b"r0[gid]", 0, 9, 7, None, 0, "OUT")),
          cnt(100, [101, 102, 103], [], hits=104))
    # missing keys are zeros, device RNG, launch 0; an empty expression goes over as an empty string
    got = dev.step_fused(0.5, {"n_expr": ""}, ROWS)
    assert owned(got) and type(got["N"]) is int and type(got["hits"]) is int
    check(dev, got,
          ("pcl_step_fused", (None, 0.5, 1, 0.0, 0.0, 0, 0.0, 0.0, b"", 1, 0, 0, FLAT, 2, "OUT")),
          cnt(100, [101, 102, 103], [104, 105], hits=106))
    for planes in (READY, FORTRAN, tuple(map(tuple, ROWS)), np.array(FLAT, dtype=np.float32)):
        check(dev, dev.step_fused(0.5, {"A": 2}, planes),
              ("pcl_step_fused", (None, 0.5, 1, 2.0, 0.0, 0, 0.0, 0.0, None, 1, 0, 0, FLAT, 2, "OUT")),
              cnt(100, [101, 102, 103], [104, 105], hits=106))
    check(dev, dev.step_fused(0.5, None, READY, sync=False, lazy=True),
          ("pcl_step_fused", (None, 0.5, 0, 0.0, 0.0, 4, 0.0, 0.0, None, 1, 0, 0, FLAT, 2, None)), None)
    check(dev, dev.step_fused(0.5, {"step": -1}, None, sync=False),
          ("pcl_step_fused", (None, 0.5, 1, 0.0, 0.0, 0, 0.0, 0.0, None, 1, 0, 0xFFFFFFFF, None, -1, None)), None)


def test_step_fused_read(dev):
    check(dev, dev.step_fused_read(), ("pcl_step_fused_read", (None, 0, "OUT")), cnt(100, [101, 102, 103], [], hits=104))
    got = dev.step_fused_read(2)
    assert owned(got) and type(got["N"]) is int and type(got["hits"]) is int
    check(dev, got, ("pcl_step_fused_read", (None, 2, "OUT")), cnt(100, [101, 102, 103], [104, 105], hits=106))


# ------------------------------------------------------------------------------------------------ Device.step_fused_multi
def test_step_fused_multi(dev):
    with pytest.raises(KeyError):
        dev.step_fused_multi(0.5, 2, {"n": 1.0})
    with pytest.raises(KeyError):
        dev.step_fused_multi(0.5, 2, {"A": 1.0})
    assert dev.lib.calls == []
    got = dev.step_fused_multi(1, 2, {"A": 1, "n": 2})
    assert owned(got) and type(got) is list and type(got[1]["N"]) is int and type(got[1]["hits"]) is int
    check(dev, got,
          ("pcl_step_fused_multi", (None, 1.0, 2, 1.0, 2.0, 0, 0.0, 0.0, None, 0, 0, None, 0, "OUT")),
          [cnt(100, [101, 102, 103], [], hits=104), cnt(105, [106, 107, 108], [], hits=109)])
    # (rng_mode is not an argument of this entry point: the device RNG always)
    for planes in (ROWS, READY, FORTRAN):
        got = dev.step_fused_multi(0.5, 2, FULL, planes)
        assert owned(got)
        check(dev, got,
              ("pcl_step_fused_multi", (None, 0.5, 2, 1.0, 2.5, 3, 4.0, 5.5, b"r0[gid]", 9, 7, FLAT, 2, "OUT")),
              [cnt(100, [101, 102, 103], [104, 105], hits=106), cnt(107, [108, 109, 110], [111, 112], hits=113)])
    got = dev.step_fused_multi(0.5, 3, {"A": 1, "n": 2, "n_expr": ""}, READY[:1], raw=True)
    assert got.base is None
    check(dev, got,
          ("pcl_step_fused_multi", (None, 0.5, 3, 1.0, 2.0, 0, 0.0, 0.0, b"", 0, 0, [1.0, 2.0, 3.0], 1, "OUT")),
          np.array([[100, 101, 102, 103, 104, 105], [106, 107, 108, 109, 110, 111], [112, 113, 114, 115, 116, 117]], dtype=I8))
    for raw in (False, True):
        check(dev, dev.step_fused_multi(0.5, 2, {"A": 1, "n": 2, "step": BIG}, (), sync=False, raw=raw),
              ("pcl_step_fused_multi", (None, 0.5, 2, 1.0, 2.0, 0, 0.0, 0.0, None, 0, 11, None, 0, None)), None)


# ------------------------------------------------------------------------------------------------ Device.step_mixed_multi
def test_step_mixed_multi(dev):
    with pytest.raises(KeyError):
        dev.step_mixed_multi(0.5, 1, ("iso", "newton"))
    assert dev.lib.calls == []
    got = dev.step_mixed_multi(1, 2, ("iso", "delete"))
    assert owned(got) and type(got) is list and type(got[0]["N"]) is int and type(got[0]["hits"]) is int and \
        type(got[1]["removed"]) is int
    check(dev, got,
          ("pcl_step_mixed_multi", (None, 1.0, 2, 2, [0, 1], 0.0, 0.0, 0, 0.0, 0.0, None, 0.0, 0.0, 0, 0, None, 0, "OUT")),
          [cnt(100, [101, 102, 103], [], "iso", hits=104), cnt(105, [106, 107, 108], [], "delete", removed=109),
           cnt(110, [111, 112, 113], [], "iso", hits=114), cnt(115, [116, 117, 118], [], "delete", removed=119)])
    for planes in (ROWS, READY, FORTRAN):
        got = dev.step_mixed_multi(0.5, 1, ["delete", "iso"], FULL, (0.25, 1), planes, 5, BIG)
        assert owned(got)
        # (the dict's own rng_mode / seed / step are not read here: seed and step are arguments)
        check(dev, got,
              ("pcl_step_mixed_multi", (None, 0.5, 1, 2, [1, 0], 1.0, 2.5, 3, 4.0, 5.5, b"r0[gid]", 0.25, 1.0, 5, 11, FLAT, 2,
                                        "OUT")),
              [cnt(100, [101, 102, 103], [104, 105], "delete", removed=106),
               cnt(107, [108, 109, 110], [111, 112], "iso", hits=113)])
    got = dev.step_mixed_multi(0.5, 2, ("delete",), {"n_expr": ""}, None, READY[1:], raw=True)
    assert got.base is None
    check(dev, got,
          ("pcl_step_mixed_multi", (None, 0.5, 2, 1, [1], 0.0, 0.0, 0, 0.0, 0.0, b"", 0.0, 0.0, 0, 0, [4.0, 5.0, 6.0], 1,
                                    "OUT")),
          np.array([[100, 101, 102, 103, 104, 105], [106, 107, 108, 109, 110, 111]], dtype=I8))


# ------------------------------------------------------------------------------------------------ Device.trace_ahead
def test_trace_ahead(dev):
    block = (100.0 + np.arange(16)).reshape(2, 2, 4)
    check(dev, dev.trace_ahead([3, 1], 1, 2, ("delete",)),
          ("pcl_store_trace_ahead", (None, [3, 1], 2, 1.0, 2, 1, [1], 0, 0.0, 0.0, 0, 0.0, 0.0, None, 0.0, 0.0, 0, 0, "OUT")),
          block)
    check(dev, dev.trace_ahead(np.array([3, 1], dtype=np.int32), 0.5, 2, ["iso", "delete"], 1, FULL, (0.25, 1), 5, BIG),
          ("pcl_store_trace_ahead", (None, [3, 1], 2, 0.5, 2, 2, [0, 1], 1, 1.0, 2.5, 3, 4.0, 5.5, b"r0[gid]", 0.25, 1.0, 5, 11,
                                     "OUT")),
          block)
    with pytest.raises(KeyError):
        dev.trace_ahead([0], 0.5, 1, ("both",))
    assert dev.lib.calls == []
    # deferred: the launch gets no host buffer, the rows come with pcl_store_trace_read
    read = dev.trace_ahead([3, 1], 0.5, 2, ("iso",), 0, {"n_expr": ""}, defer=True)
    assert callable(read)
    check(dev, None,
          ("pcl_store_trace_ahead", (None, [3, 1], 2, 0.5, 2, 1, [0], 0, 0.0, 0.0, 0, 0.0, 0.0, b"", 0.0, 0.0, 0, 0, None)),
          None)
    check(dev, read(), ("pcl_store_trace_read", (None, "OUT", 16)), block)
    # ... unless nothing is tracked: then there is nothing to read later
    read = dev.trace_ahead([], 0.5, 2, ("iso",), defer=True)
    check(dev, None,
          ("pcl_store_trace_ahead", (None, [], 0, 0.5, 2, 1, [0], 0, 0.0, 0.0, 0, 0.0, 0.0, None, 0.0, 0.0, 0, 0, "OUT")), None)
    got = read()
    assert dev.lib.calls == [] and got.shape == (2, 0, 4) and got.dtype == F8


# ------------------------------------------------------------------------------------------------ Device.step_fused_delete
def test_step_fused_delete(dev):
    got = dev.step_fused_delete(1, 2, 3)
    assert type(got["N"]) is int and type(got["removed"]) is int
    check(dev, got, ("pcl_step_fused_delete", (None, 1.0, 2.0, 3.0, 0, 1, 0, 0, None, -1, "OUT")),
          cnt(100, [101, 102, 103], [], removed=104))
    check(dev, dev.step_fused_delete(0.5, 0.25, 2.5, 0, 9, BIG, (), lazy=True),
          ("pcl_step_fused_delete", (None, 0.5, 0.25, 2.5, 4, 0, 9, 11, None, 0, "OUT")),
          cnt(100, [101, 102, 103], [], removed=104))
    for planes in (ROWS, READY, FORTRAN, READY.reshape(-1)):
        got = dev.step_fused_delete(0.5, 0.25, 2.5, planes=planes)
        # the answer's arrays are views of the call's own buffer (the host-latency path of the delete loop: no copies)
        assert got["sign"].base is not None and got["sign"].base is got["planes"].base
        check(dev, got, ("pcl_step_fused_delete", (None, 0.5, 0.25, 2.5, 0, 1, 0, 0, FLAT, 2, "OUT")),
              cnt(100, [101, 102, 103], [104, 105], removed=106))
    first = dev.step_fused_delete(0.5, 0.25, 2.5, planes=READY)
    again = dev.step_fused_delete(0.5, 0.25, 2.5, planes=READY)
    assert not np.shares_memory(first["sign"], again["sign"]) and not np.shares_memory(first["planes"], again["planes"])


def test_step_fused_delete_multi(dev):
    got = dev.step_fused_delete_multi(1, 2, 2, 3)
    assert owned(got) and type(got) is list and type(got[1]["N"]) is int and type(got[1]["removed"]) is int
    check(dev, got, ("pcl_step_fused_delete_multi", (None, 1.0, 2, 2.0, 3.0, 0, 0, None, -1, "OUT")),
          [cnt(100, [101, 102, 103], [], removed=104), cnt(105, [106, 107, 108], [], removed=109)])
    check(dev, dev.step_fused_delete_multi(0.5, 1, 0.25, 2.5, 9, BIG, ()),
          ("pcl_step_fused_delete_multi", (None, 0.5, 1, 0.25, 2.5, 9, 11, None, 0, "OUT")),
          [cnt(100, [101, 102, 103], [], removed=104)])
    for planes in (ROWS, READY, FORTRAN):
        got = dev.step_fused_delete_multi(0.5, 2, 0.25, 2.5, planes=planes)
        assert owned(got)
        check(dev, got, ("pcl_step_fused_delete_multi", (None, 0.5, 2, 0.25, 2.5, 0, 0, FLAT, 2, "OUT")),
              [cnt(100, [101, 102, 103], [104, 105], removed=106), cnt(107, [108, 109, 110], [111, 112], removed=113)])
    for planes, flat, n_planes, rows in ((None, None, -1, [[100, 101, 102, 103, 104], [105, 106, 107, 108, 109]]),
                                         (READY[:1], [1.0, 2.0, 3.0], 1, [[100, 101, 102, 103, 104, 105],
                                                                          [106, 107, 108, 109, 110, 111]])):
        got = dev.step_fused_delete_multi(0.5, 2, 0.25, 2.5, 9, 7, planes, raw=True)
        assert got.base is None
        check(dev, got, ("pcl_step_fused_delete_multi", (None, 0.5, 2, 0.25, 2.5, 9, 7, flat, n_planes, "OUT")),
              np.array(rows, dtype=I8))


def test_step_counters(dev):
    check(dev, dev.step_counters(), ("pcl_step_counters", (None, None, 0, "OUT")), np.array([100, 101, 102, 103], dtype=I8))
    for planes in (ROWS, READY, FORTRAN):
        got = dev.step_counters(planes)
        assert got.base is None
        check(dev, got, ("pcl_step_counters", (None, FLAT, 2, "OUT")), np.array([100, 101, 102, 103, 104, 105], dtype=I8))
    with pytest.raises(ValueError):
        dev.step_counters(None)                      # the counters cannot be "off" here
    assert dev.lib.calls == []


# ------------------------------------------------------------------------------------------------ DeviceGroup
def test_group_step_fused_multi(grp):
    with pytest.raises(KeyError):
        grp.step_fused_multi(0.5, 2, {"n": 1.0})
    assert grp.lib.calls == []
    got = grp.step_fused_multi(1, 2, {"A": 1, "n": 2})
    assert got.base is None
    check(grp, got, ("pcl_group_step_fused_multi", (None, 1.0, 2, 1.0, 2.0, 0, 0.0, 0.0, None, 0, 0, None, 0, "OUT")),
          np.array([[100, 101, 102, 103, 104], [105, 106, 107, 108, 109]], dtype=I8))
    for planes in (ROWS, READY, FORTRAN):
        check(grp, grp.step_fused_multi(0.5, 1, FULL, planes),
              ("pcl_group_step_fused_multi", (None, 0.5, 1, 1.0, 2.5, 3, 4.0, 5.5, b"r0[gid]", 9, 7, FLAT, 2, "OUT")),
              np.array([[100, 101, 102, 103, 104, 105, 106]], dtype=I8))
    # the group binding hands an empty expression over as NULL (Device hands over the empty string)
    check(grp, grp.step_fused_multi(0.5, 1, {"A": 1, "n": 2, "n_expr": "", "step": BIG}),
          ("pcl_group_step_fused_multi", (None, 0.5, 1, 1.0, 2.0, 0, 0.0, 0.0, None, 0, 11, None, 0, "OUT")),
          np.array([[100, 101, 102, 103, 104]], dtype=I8))


def test_group_step_fused_delete(grp):
    got = grp.step_fused_delete(1, 2, 3, 9, BIG)
    assert got.base is None
    check(grp, got, ("pcl_group_step_fused_delete", (None, 1.0, 2.0, 3.0, 4, 1, 9, 11, None, 0, "OUT")),
          np.array([100, 101, 102, 103, 104], dtype=I8))
    for planes in (ROWS, READY, FORTRAN):
        check(grp, grp.step_fused_delete(0.5, 0.25, 2.5, 9, 7, planes, lazy=False),
              ("pcl_group_step_fused_delete", (None, 0.5, 0.25, 2.5, 0, 1, 9, 7, FLAT, 2, "OUT")),
              np.array([100, 101, 102, 103, 104, 105, 106], dtype=I8))


def test_group_step_fused_delete_multi(grp):
    check(grp, grp.step_fused_delete_multi(1, 2, 2, 3, 9, BIG),
          ("pcl_group_step_fused_delete_multi", (None, 1.0, 2, 2.0, 3.0, 9, 11, None, 0, "OUT")),
          np.array([[100, 101, 102, 103, 104], [105, 106, 107, 108, 109]], dtype=I8))
    for planes in (ROWS, READY, FORTRAN):
        got = grp.step_fused_delete_multi(0.5, 1, 0.25, 2.5, 9, 7, planes)
        assert got.base is None
        check(grp, got, ("pcl_group_step_fused_delete_multi", (None, 0.5, 1, 0.25, 2.5, 9, 7, FLAT, 2, "OUT")),
              np.array([[100, 101, 102, 103, 104, 105, 106]], dtype=I8))


def test_group_step_mixed_multi(grp):
    with pytest.raises(KeyError):
        grp.step_mixed_multi(0.5, 1, ("iso", "newton"), {}, (0, 0), 0, 0)
    assert grp.lib.calls == []
    check(grp, grp.step_mixed_multi(1, 2, ("iso", "delete"), {"n_expr": ""}, (1, 0.25), 9, BIG),
          ("pcl_group_step_mixed_multi", (None, 1.0, 2, 2, [0, 1], 0.0, 0.0, 0, 0.0, 0.0, None, 1.0, 0.25, 9, 11, None, 0,
                                          "OUT")),
          (100 + np.arange(20, dtype=I8)).reshape(4, 5))
    for planes in (ROWS, READY, FORTRAN):
        got = grp.step_mixed_multi(0.5, 1, ["delete"], FULL, (1, 0.25), 9, 7, planes)
        assert got.base is None
        check(grp, got,
              ("pcl_group_step_mixed_multi", (None, 0.5, 1, 1, [1], 1.0, 2.5, 3, 4.0, 5.5, b"r0[gid]", 1.0, 0.25, 9, 7, FLAT, 2,
                                              "OUT")),
              np.array([[100, 101, 102, 103, 104, 105, 106]], dtype=I8))
