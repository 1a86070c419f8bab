"""One launcher for the tests that need a world of ranks: ``run_world(worker_source, world)`` runs the script once per rank
in fresh interpreters (never a re-exec of the caller), each with ``physicl_amd.launch.rank_env`` on a free port, and returns
what each rank printed last, as JSON, in rank order.  Whatever way it ends -- a rank failed, the time ran out, an exception
-- exactly the processes started here are stopped before it returns: a rank whose sibling died would otherwise sit in its
collective, with the GPU open, until somebody's time limit."""
import json
import os
import subprocess
import sys
import tempfile
import time

from physicl_amd import launch


def run_world(worker_source, world, timeout=600.0, grace_s=5.0):
    port, parent = launch.free_port(), os.getpid()
    procs, files = [], []
    failure = None
    try:
        for r in range(world):
            # (files, not pipes: nobody reads while the ranks run, and a rank's JSON line may be longer than a pipe holds)
            files.append((tempfile.TemporaryFile("w+"), tempfile.TemporaryFile("w+")))
            procs.append(subprocess.Popen([sys.executable, "-c", worker_source], env=launch.rank_env(os.environ, r, world, port),
                                          preexec_fn=lambda: launch._die_with_parent(parent), stdout=files[r][0], stderr=files[r][1]))
        t_end = time.time() + timeout
        while failure is None:
            states = [p.poll() for p in procs]
            bad = [r for r, s in enumerate(states) if s not in (None, 0)]
            if bad:                                      # the others are not waited for: they are stopped below, at once
                failure = "rank %d of %d exited with %d" % (bad[0], world, states[bad[0]])
            elif all(s == 0 for s in states):
                break
            elif time.time() > t_end:
                bad = [r for r, s in enumerate(states) if s is None]
                failure = "rank %d of %d was still running after %g s" % (bad[0], world, timeout)
            else:
                time.sleep(0.02)
    finally:
        launch._stop(procs, grace_s)
        texts = []
        for pair in files:
            for f in pair:
                f.seek(0)
            texts.append([f.read() for f in pair])       # (closing a temporary file removes it)
            for f in pair:
                f.close()
    if failure is not None:
        raise AssertionError("%s; its stderr ends:\n%s" % (failure, texts[bad[0]][1][-3000:]))
    return [json.loads(out.strip().splitlines()[-1]) for out, _ in texts]
