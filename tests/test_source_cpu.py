"""CPU: photon sources for bulk generation (light.PhotonSource, generate_photons_bulk(..., source=)) without a GPU.

* the constructor's refusals and the frame it makes;
* ``generate_photons_bulk`` keeps its parameters in place, ``source`` comes last and combines with every energy form;
* what ``Device.apply_source`` / ``DeviceGroup.apply_source`` put over the C ABI, on a stand-in for the library in the manner of
  tests/test_spectrum_cpu.py; ``Simulation._upload_locked`` on a stand-in device fills, then applies the source once -- and makes no
  such call without a source;
* the numpy restatement of the draws (tests/source_reference.py) meets the distributions' own 5-sigma conditions at n = 2^20:
  what the GPU tests compare the device against is itself a sampler of the right distributions.

The unit's build is held in tests/test_build_cpu.py.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import physicl_amd as phys
from physicl_amd import _hip, build, light
from source_reference import check_cone, check_disc, check_gaussian, check_isotropic, check_lambertian, source_state

SEED = 0x5EED50C5
N_STAT = 1 << 20
C = float(np.asarray(light.c))


# ------------------------------------------------------------------------------------------------ constructor
@pytest.mark.parametrize("kw", [
    dict(direction=(0, 0, 0)), dict(direction=(1, np.nan, 0)), dict(direction=(1, np.inf, 0)), dict(direction=(1, 0)),
    dict(origin=(0, np.inf, 0)), dict(origin=(1, 2)), dict(origin="abc"),
    dict(angular="laser"), dict(spatial="line"),
    dict(angular="cone"), dict(angular="cone", half_angle=0.0), dict(angular="cone", half_angle=-0.1), dict(angular="cone", half_angle=3.2),
    dict(angular="cone", half_angle=np.nan), dict(angular="beam", half_angle=0.3), dict(angular="isotropic", half_angle=0.3),
    dict(angular="lambertian", half_angle=0.3),
    dict(spatial="disc"), dict(spatial="gaussian"), dict(spatial="disc", radius=0.0), dict(spatial="disc", radius=-1.0),
    dict(spatial="gaussian", radius=np.inf), dict(spatial="gaussian", radius=np.nan), dict(spatial="point", radius=1.0)])
def test_malformed_sources_are_refused_at_construction(kw):
    with pytest.raises(ValueError):
        light.PhotonSource(**kw)


def test_defaults_and_accepted_forms():
    s = light.PhotonSource()
    assert s.origin.tolist() == [0, 0, 0] and s.d.tolist() == [1, 0, 0] and s.angular == "beam" and s.spatial == "point"
    assert light.PhotonSource(angular="cone", half_angle=np.pi).cos_half_angle == -1.0
    m = light.PhotonSource(origin=light.Measurement([6371000, 0, 0], "m**1"), spatial="disc", radius=light.Measurement(2.5, "m**1"))
    assert m.origin.dtype == np.float64 and type(m.origin) is np.ndarray and m.radius == 2.5 * float(np.asarray(light.Measurement(1, "m**1")))
    assert m.origin[0] == float(np.asarray(light.Measurement(6371000, "m**1")))      # taken in code units, like min / max


AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


@pytest.mark.parametrize("direction", AXES + [(1, -2, 0.5), (3, 3, 3), (1e-9, 2e-9, -1e-9), (-5e8, 1, 1), (0, 1, 1), (2, 0, -2), (0.1, 0.1, 7)])
def test_frame_is_orthonormal_and_right_handed(direction):
    s = light.PhotonSource(direction=direction)
    F = np.stack([s.e1, s.e2, s.d])
    assert np.max(np.abs(F @ F.T - np.eye(3))) <= 4e-16
    assert np.max(np.abs(np.cross(s.e1, s.e2) - s.d)) <= 4e-16          # right-handed: e1 x e2 = d
    dn = np.asarray(direction, dtype=np.float64)
    assert np.max(np.abs(s.d - dn / np.linalg.norm(dn))) <= 4e-16
    if direction in AXES:                                                 # exact unit vectors, no negative zeros
        for vec in (s.e1, s.e2, s.d):
            assert sorted(np.abs(vec).tolist()) == [0.0, 0.0, 1.0] and not np.any(np.signbit(vec) & (vec == 0))
        assert s.d.tolist() == list(direction)


def test_the_frame_s_helper_axis_is_the_smallest_component_lowest_index_on_a_tie():
    assert light.PhotonSource(direction=(1, 0, 0)).e1.tolist() == [0, 0, -1]       # a = y: (0,1,0) x (1,0,0)
    assert light.PhotonSource(direction=(0, 0, -1)).e1.tolist() == [0, 1, 0]       # a = x: (1,0,0) x (0,0,-1)
    s = light.PhotonSource(direction=(1, -2, 0.5))
    assert s.e1[2] == 0.0 and s.e1[0] > 0                                            # a = z


# ------------------------------------------------------------------------------------------------ generate_photons_bulk
def test_signature_keeps_its_parameters_in_place_with_source_last():
    params = list(inspect.signature(light.generate_photons_bulk).parameters.values())
    assert [p.name for p in params] == ["n", "min", "max", "seed", "T", "bins", "fn_vec", "source"]
    assert params[-1].default is None
    params = list(inspect.signature(phys.PhotonBatch.__init__).parameters.values())
    assert [p.name for p in params] == ["self", "n", "e_min", "e_max", "seed", "table", "fn_vec", "source"] and params[-1].default is None


def test_source_combines_with_every_energy_form():
    src = light.PhotonSource(origin=(6371000, 0, 0), angular="isotropic")
    plain = light.generate_photons_bulk(10, min=1.0, max=2.0, seed=3, source=src)
    planck = light.generate_photons_bulk(10, min=1e-19, max=9e-19, seed=3, T=5800.0, bins=100, source=src)
    fn = lambda size: np.full(size, 0.5)                                                                     # noqa: E731
    sampled = light.generate_photons_bulk(10, min=1.0, max=2.0, seed=3, fn_vec=fn, source=src)
    assert plain.source is src and planck.source is src and sampled.source is src
    assert plain.table is None and planck.table is not None and sampled.fn_vec is fn
    assert light.generate_photons_bulk(10, min=1.0, max=2.0).source is None
    with pytest.raises(ValueError):
        light.generate_photons_bulk(10, min=1.0, max=2.0, source="isotropic")


# ------------------------------------------------------------------------------------------------ binding
class FakeLib:
    """Records the call with a copy of the structure behind its pointer."""

    def __init__(self):
        self.calls = []

    def _apply(self, name, handle, src, c, seed):
        st = _hip.SourceStruct.from_address(src)
        self.calls.append((name, handle, {f: (list(getattr(st, f)) if f in ("origin", "e1", "e2", "d") else getattr(st, f)) for f, _ in st._fields_},
                           c, seed))
        return 0

    def pcl_store_apply_source(self, *a):
        return self._apply("pcl_store_apply_source", *a)

    def pcl_group_apply_source(self, *a):
        return self._apply("pcl_group_apply_source", *a)


@pytest.mark.parametrize("cls,handle,entry", [(_hip.Device, "ctx", "pcl_store_apply_source"), (_hip.DeviceGroup, "g", "pcl_group_apply_source")])
def test_apply_source_marshalling(cls, handle, entry):
    d = cls.__new__(cls)
    d.lib = FakeLib()
    setattr(d, handle, None)
    src = light.PhotonSource(origin=(6371000, -2, 0.5), direction=(1, -2, 0.5), angular="cone", half_angle=0.3, spatial="gaussian", radius=7.5)
    d.apply_source(src, C, 2 ** 40 + 17)
    (name, h, st, c, seed), = d.lib.calls
    assert name == entry and h is None and c == C and seed == 2 ** 40 + 17
    assert st["origin"] == [6371000.0, -2.0, 0.5] and st["e1"] == src.e1.tolist() and st["e2"] == src.e2.tolist() and st["d"] == src.d.tolist()
    assert st["angular"] == 2 and st["spatial"] == 2 and st["cos_half_angle"] == float(np.cos(0.3)) and st["radius"] == 7.5
    d.apply_source(light.PhotonSource(angular="lambertian", spatial="disc", radius=1.0), C, 0)
    assert (d.lib.calls[1][2]["angular"], d.lib.calls[1][2]["spatial"]) == (3, 1)
    d.apply_source(light.PhotonSource(angular="isotropic"), C, 0)
    assert (d.lib.calls[2][2]["angular"], d.lib.calls[2][2]["spatial"]) == (1, 0)


def test_structure_layout_and_prototypes():
    assert "pcl_store_apply_source" in _hip.EXPORTS and "pcl_group_apply_source" in _hip.EXPORTS
    assert len(_hip._PROTOTYPES["pcl_store_apply_source"]) == 4
    S = _hip.SourceStruct                                              # 12 doubles, 2 ints, 2 doubles: no padding in C either
    assert ctypes.sizeof(S) == 12 * 8 + 2 * 4 + 2 * 8 and S.angular.offset == 96 and S.cos_half_angle.offset == 104
    header = open(os.path.join(os.path.dirname(build.HERE), "include", "physicl_hip.h")).read()
    for name, table in (("PCL_SRC_BEAM", 0), ("PCL_SRC_ISOTROPIC", 1), ("PCL_SRC_CONE", 2), ("PCL_SRC_LAMBERTIAN", 3), ("PCL_SRC_POINT", 0),
                        ("PCL_SRC_DISC", 1), ("PCL_SRC_GAUSSIAN", 2)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == table
    assert _hip.SRC_ANGULAR == {"beam": 0, "isotropic": 1, "cone": 2, "lambertian": 3} and _hip.SRC_SPATIAL == {"point": 0, "disc": 1, "gaussian": 2}


class FakeDevice:
    np_dtype = np.float64

    def __init__(self):
        self.capacity, self.calls = 0, []

    def store_alloc(self, n):
        self.capacity = n
        self.calls.append(("store_alloc", n))

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a: self.calls.append((name,) + a)


def upload(batch):
    sim = phys.Simulation(cl_on=False)
    sim.add_objs(batch)
    sim._hip = _hip
    dev = FakeDevice()
    sim._upload_locked(dev)
    return dev.calls


def test_upload_fills_then_applies_the_source_once():
    src = light.PhotonSource(origin=(6371000, 0, 0), angular="isotropic")
    calls = upload(light.generate_photons_bulk(100, min=1.0, max=2.0, seed=9, source=src))
    assert [c[0] for c in calls] == ["store_alloc", "fill_photons", "apply_source"]
    assert calls[1][1:] == (100, 0, C, 1.0, 2.0, 9) and calls[2][1] is src and calls[2][2:] == (C, 9)
    calls = upload(light.generate_photons_bulk(100, min=1e-19, max=9e-19, seed=9, T=5800.0, bins=50, source=src))
    assert [c[0] for c in calls] == ["store_alloc", "fill_photons_table", "apply_source"] and calls[2][1:] == (src, C, 9)
    calls = upload(light.generate_photons_bulk(100, min=1.0, max=2.0, seed=9, fn_vec=lambda size: np.full(size, 0.25), source=src))
    assert [c[0] for c in calls] == ["store_alloc", "fill_photons", "upload", "apply_source"] and calls[3][1:] == (src, C, 9)


def test_upload_without_a_source_makes_no_extra_call():
    assert [c[0] for c in upload(light.generate_photons_bulk(100, min=1.0, max=2.0, seed=9))] == ["store_alloc", "fill_photons"]
    assert [c[0] for c in upload(light.generate_photons_bulk(100, min=1e-19, max=9e-19, seed=9, T=5800.0, bins=50))] == ["store_alloc", "fill_photons_table"]
    fn = lambda size: np.full(size, 0.25)                                                                    # noqa: E731
    assert [c[0] for c in upload(light.generate_photons_bulk(100, min=1.0, max=2.0, seed=9, fn_vec=fn))] == ["store_alloc", "fill_photons", "upload"]


def test_multidevice_applies_the_source_on_every_shard():
    from physicl_amd.multidev import MultiDevice
    md = MultiDevice.__new__(MultiDevice)
    md.shards = [FakeDevice(), FakeDevice()]
    from concurrent.futures import ThreadPoolExecutor
    md._pool = ThreadPoolExecutor(max_workers=2)
    src = light.PhotonSource(angular="isotropic")
    md.apply_source(src, C, 4)
    md._pool.shutdown()
    assert [s.calls for s in md.shards] == [[("apply_source", src, C, 4)]] * 2


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.fixture(scope="module")
def ids():
    return np.arange(N_STAT, dtype=np.uint64)


def test_restatement_isotropic(ids):
    st = source_state(light.PhotonSource(direction=(1, -2, 0.5), angular="isotropic"), ids, SEED, C)
    check_isotropic(st["v"] / C)
    assert np.max(np.abs(np.sqrt(np.sum((st["v"] / C) ** 2, axis=1)) - 1.0)) <= 1e-15
    assert st["mu"].min() < -0.999 and st["mu"].max() > 0.999 and st["rho"] is None


def test_restatement_cone(ids):
    st = source_state(light.PhotonSource(direction=(0, 0, -1), angular="cone", half_angle=0.3), ids, SEED, C)
    check_cone(st["mu"], 0.3)
    check_cone(st["v"][:, 2] / -C, 0.3)                                  # the same from the velocities: mu = v . d / c


def test_restatement_lambertian(ids):
    st = source_state(light.PhotonSource(direction=(0, 1, 0), angular="lambertian"), ids, SEED, C)
    check_lambertian(st["mu"])
    check_lambertian(st["v"][:, 1] / C)


def test_restatement_disc_and_gaussian(ids):
    origin = np.array([6371000.0, 0.0, 0.0])
    st = source_state(light.PhotonSource(origin=origin, direction=(1, 0, 0), spatial="disc", radius=2.5), ids, SEED, C)
    check_disc(st["rho"], 2.5)
    off = st["r"] - origin
    assert np.all(off[:, 0] == 0) and np.all(st["v"] == [C, 0, 0])      # in the plane perpendicular to d; a beam is a constant
    st = source_state(light.PhotonSource(direction=(0, 0, 1), spatial="gaussian", radius=3.0), ids, SEED, C)
    check_gaussian(st["rho"], 3.0)
    check_gaussian(np.hypot(st["r"][:, 0], st["r"][:, 1]), 3.0)
    assert np.all(np.isfinite(st["r"])) and st["rho"].max() <= 3.0 * 9.0  # sqrt(-2 ln 2^-53) < 9


def test_restatement_does_not_depend_on_the_shard():
    src = light.PhotonSource(origin=(1, 2, 3), direction=(1, -2, 0.5), angular="lambertian", spatial="gaussian", radius=2.0)
    whole = source_state(src, np.arange(5000), SEED, C)
    part = source_state(src, np.arange(4097, 5000), SEED, C)
    assert np.array_equal(whole["r"][4097:], part["r"]) and np.array_equal(whole["v"][4097:], part["v"])
    other = source_state(src, np.arange(5000), SEED + 1, C)
    assert not np.array_equal(whole["v"], other["v"])
