"""CPU: the six steps that write the store share one host scaffold, ``tally.WriterStep`` -- "refuse -> prepare -> move the pass
counter -> one sweep -> one collective -> record", on the device and on host-resident objects.  What each step computes is held in
its own test file; here: the steps are on the base, carry no ``run`` / ``_device_run`` of their own, and a call that is
refused -- by the step's own rule or by a hook that raises -- leaves the step as it was."""
import numpy as np
import pytest

import physicl as phys
import physicl.light
from physicl_amd import light, tally

C = light._c_h_literals()[0]
STEPS = {
    "SurfaceReflectStep": lambda: phys.light.SurfaceReflectStep(2.0, albedo=0.5),
    "PhaseFunctionStep": lambda: phys.light.PhaseFunctionStep("hg", 0.85),
    "AbsorptionStep": lambda: phys.light.AbsorptionStep(0.5),
    "LayeredPhaseStep": lambda: phys.light.LayeredPhaseStep(["rayleigh"]),
    "RecycleStep": lambda: phys.light.RecycleStep(phys.light.PhotonSource()),
    "PathAbsorptionStep": lambda: phys.light.PathAbsorptionStep(0.25),
}
# the collective of these two is their counts alone (sim._global), not tally.reduce_parts' payload behind the shard's size
OWN_COLLECTIVE = {"SurfaceReflectStep", "PhaseFunctionStep"}


def photons(n=12):
    out = []
    for k in range(n):
        o = phys.light.PhotonObject(E=phys.Measurement(np.double(1e-19), "J**1"), v=phys.light.c * [1, 0, 0])
        o.v, o.dv = np.array([C, 0.0, 0.0]), np.array([0.0, C * (k % 2), 0.0])
        out.append(o)
    return out


class HostSim:                                                         # what the host path asks of a simulation (no device here)
    _residency, _batch, comm, launch_note = "host", None, None, None
    t, seed, dt = 0.25, 7, 1e-9

    def __init__(self, py=False):
        self.objects, self.py = photons(), py

    def _py_semantics(self):
        return self.py


class DeviceSim(HostSim):                                              # ... and the device path; a sweep here would be an AttributeError
    _residency, _scattered = "device", False

    def _k_wanted(self):
        return 32

    def _dt_code(self):
        return float(self.dt)


@pytest.mark.parametrize("name", sorted(STEPS))
def test_the_step_is_on_the_base_and_keeps_only_its_hooks(name):
    cls = getattr(phys.light, name)
    assert issubclass(cls, tally.WriterStep) and cls.__mro__[1] is tally.WriterStep
    own = set(vars(cls))
    assert not own & {"run", "_device_run"}, own
    assert ("_reduce" in own) == (name in OWN_COLLECTIVE)
    assert {"_sweep", "_host_sweep", "_record_pass", "__init__", "_NOTE"} <= own
    assert cls._device_run is tally.WriterStep._device_run and cls.run is tally.WriterStep.run
    assert "one launch per light step" in cls._NOTE and name in cls._NOTE and cls._fuse_role is None


@pytest.mark.parametrize("hook", ["_refuse", "_prepare"])
@pytest.mark.parametrize("name", sorted(STEPS))
def test_a_hook_that_raises_leaves_the_step_as_it_was(name, hook, monkeypatch):
    step = STEPS[name]()

    def no(*a):
        raise ValueError("refused by " + hook)
    monkeypatch.setattr(step, hook, no)
    host, dev = HostSim(), DeviceSim()
    with pytest.raises(ValueError, match="refused by"):
        step.run(host)
    with pytest.raises(ValueError, match="refused by"):
        step._device_run(dev)
    assert step._pass == 0 and step.data == []
    assert dev.launch_note is None and not dev._scattered              # nothing was said, nothing was launched
    for o in host.objects:
        assert np.array_equal(o.v, [C, 0.0, 0.0])


@pytest.mark.parametrize("name", ["PhaseFunctionStep", "AbsorptionStep", "LayeredPhaseStep"])
def test_python_semantics_are_refused_on_both_paths(name):
    step = STEPS[name]()
    with pytest.raises(ValueError, match="cl_on=True"):
        step.run(HostSim(py=True))
    with pytest.raises(ValueError, match="cl_on=True"):
        step._device_run(DeviceSim(py=True))
    assert step._pass == 0 and step.data == []


def test_a_time_step_the_path_absorption_refuses_leaves_it_as_it_was():
    step = STEPS["PathAbsorptionStep"]()
    host, dev = HostSim(), DeviceSim()
    host.dt = dev.dt = -1e-9
    with pytest.raises(ValueError):
        step.run(host)
    with pytest.raises(ValueError):
        step._device_run(dev)
    assert step._pass == 0 and step.data == [] and dev.launch_note is None


@pytest.mark.parametrize("name", sorted(STEPS))
def test_the_host_path_moves_the_pass_counter_once_and_says_nothing(name):
    step, sim = STEPS[name](), HostSim()
    step.run(sim)
    step.run(sim)
    assert step._pass == 2 and len(step.data) == 2 and sim.launch_note is None
    assert all(type(o.v) is np.ndarray and o.v.dtype == np.float64 for o in sim.objects)
