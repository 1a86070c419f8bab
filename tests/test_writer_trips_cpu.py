"""Every sweep of the add-on units has a test that takes it past its first trip ("Trips"): the table
``TRIP_CASES`` of tests/test_writer_trips_gpu.py against the sweeps the build describes.  A sweep added without such a case fails
here, on a machine without a GPU."""
import ast
import os

from physicl_amd import build
from test_writer_trips_gpu import TRIP_CASES

TESTS = os.path.dirname(os.path.abspath(__file__))


def test_every_described_sweep_has_a_trip_case_and_no_other_kernel_is_named():
    kernels = [s["kernel"] for u in build.ADDONS for s in u["sweeps"]]
    assert len(kernels) == len(set(kernels)) == 17
    assert sorted(TRIP_CASES) == sorted(kernels)


def test_every_named_test_exists_in_the_named_file():
    for kernel, (name, test) in TRIP_CASES.items():
        path = os.path.join(TESTS, name)
        assert name.startswith("test_") and os.path.isfile(path), (kernel, name)
        with open(path) as f:
            defined = {node.name for node in ast.parse(f.read()).body if isinstance(node, ast.FunctionDef)}
        assert test.startswith("test_") and test in defined, (kernel, name, test)
