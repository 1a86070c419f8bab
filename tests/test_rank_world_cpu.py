"""CPU: the tests' own launcher (tests/rank_world.py) -- each rank's JSON in rank order; a failing rank fails the call at once,
with that rank's stderr, and no process it started outlives it.  (physicl_amd/launch.py, whose pieces it is made of, is pinned
by tests/test_launch_cpu.py.)"""
import os
import time

import pytest

from rank_world import run_world

CHILD = r"""
import json, os, sys, time
r = int(os.environ["RANK"])
open(os.path.join(%(tmp)r, "pid%%d" %% r), "w").write(str(os.getpid()))
if %(fail)r and r == 1:
    while not os.path.exists(os.path.join(%(tmp)r, "pid0")):      # (so that the test knows whom to look for)
        time.sleep(0.01)
    sys.stderr.write("rank 1 gives up: no such device\n")
    sys.exit(1)
if %(fail)r or %(hang)r:
    time.sleep(60)                        # "waits in a collective for its sibling"
print("x" * 200000)                       # more than a pipe holds, and not the last line
print(json.dumps({"rank": r, "world": os.environ["WORLD_SIZE"], "port": os.environ["MASTER_PORT"], "addr": os.environ["MASTER_ADDR"],
                  "omp": os.environ["OMP_NUM_THREADS"]}))
"""


def gone(pid):
    try:
        os.kill(pid, 0)
        return open("/proc/%d/stat" % pid).read().split()[2] == "Z"
    except (OSError, IOError):
        return True


def pids(tmp_path, world):
    return [int((tmp_path / ("pid%d" % r)).read_text()) for r in range(world)]


def test_a_world_that_succeeds_returns_the_ranks_json_in_rank_order(tmp_path):
    got = run_world(CHILD % {"tmp": str(tmp_path), "fail": False, "hang": False}, 3, timeout=60)
    assert [g["rank"] for g in got] == [0, 1, 2] and {g["world"] for g in got} == {"3"} and {g["addr"] for g in got} == {"127.0.0.1"}
    assert len({g["port"] for g in got}) == 1 and int(got[0]["port"]) > 0
    assert got[0]["omp"] == os.environ.get("OMP_NUM_THREADS", "1")           # a value the machine sets wins (rank_env's setdefault)
    assert all(gone(p) for p in pids(tmp_path, 3)) and os.getpid() not in pids(tmp_path, 3)


def test_a_failing_rank_fails_the_call_at_once_and_leaves_nothing_running(tmp_path):
    t0 = time.time()
    with pytest.raises(AssertionError, match="rank 1 of 2 exited with 1") as e:
        run_world(CHILD % {"tmp": str(tmp_path), "fail": True, "hang": False}, 2, timeout=60)
    assert time.time() - t0 < 10          # rank 0, asleep for a minute, was stopped, not waited for
    assert "rank 1 gives up: no such device" in str(e.value)
    assert all(gone(p) for p in pids(tmp_path, 2))


def test_the_time_limit_fails_the_call(tmp_path):
    t0 = time.time()
    with pytest.raises(AssertionError, match="rank 0 of 2 was still running after 0 s"):      # (no limit is waited for here)
        run_world(CHILD % {"tmp": str(tmp_path), "fail": False, "hang": True}, 2, timeout=0.0)
    assert time.time() - t0 < 10
