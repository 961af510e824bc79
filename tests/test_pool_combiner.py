"""The drop-in pools' flat combiner on the CPU (no device): the stand-alone
tools/pool_combiner_check over lpcnet_amd/csrc/pool_combiner.cpp with a fake
launch -- 16 threads x 2000 calls in each of the three wake-up / gather-window
modes that tests/test_gpu_dropin.py runs on the device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_request_runs_once_and_the_pool_ends_free():
    """Exit status 0: every call returned its own rc and message and a fresh
    result, no launch overlapped another or a slot I/O or mixed shapes, the
    requests ran exactly once each, inbox / busy / arrivals ended empty, and
    no call hung (the program's own watchdog)."""
    exe = os.path.join(ROOT, "tools", "pool_combiner_check")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "tools/pool_combiner_check"], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "pool_combiner_check ok: 16 threads x 2000 calls x 3 modes" in r.stdout, r.stdout
