"""TEST INFRASTRUCTURE: the one place that knows the libraries under test -- where the simulations of tests/hostsim lie and how they are
built and loaded, what makes the HIP library the real one, the pytest fixtures for them (a test module imports the ones it uses:
``from libs import sim, wavesim  # noqa: F401``), and how a check that runs as a child process is started and read."""
import functools
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HOSTSIM_SO = ROOT / "tests" / "hostsim" / "_build" / "liblamejs_hostsim.so"      # the kernel bodies with one lane
WAVESIM_SO = ROOT / "tests" / "hostsim" / "_build" / "liblamejs_wavesim.so"      # ... with the 64 lanes of a wave as fibers
NODE = shutil.which("node")
ADDON = ROOT / "lamejs_amd" / "js" / "addon" / "lhip_napi.node"


@functools.lru_cache(maxsize=None)
def build_sims():
    """`make all` in tests/hostsim, once per process."""
    subprocess.run(["make", "-C", str(ROOT / "tests" / "hostsim"), "all"], check=True, capture_output=True)


@functools.lru_cache(maxsize=None)
def sim_library(kind):
    """The simulation ``hostsim`` or ``wavesim``, built if need be and loaded with the package's signatures."""
    import lamejs_amd
    build_sims()
    lib = lamejs_amd.load_library({"hostsim": HOSTSIM_SO, "wavesim": WAVESIM_SO}[kind])
    assert b"HOST SIMULATION" in lib.lhip_version()
    return lib


def gpu_library():
    """The HIP library on a machine with a device: never a simulation."""
    import lamejs_amd
    lib = lamejs_amd.load_library()
    assert lib.lhip_device_count() > 0, "no HIP device"
    assert b"HIP gfx950" in lib.lhip_version() and b"HOST SIMULATION" not in lib.lhip_version()
    return lib


@pytest.fixture(scope="session")
def sim():
    return sim_library("hostsim")


@pytest.fixture(scope="session")
def wavesim():
    return sim_library("wavesim")


@pytest.fixture(scope="session")
def lib():
    return gpu_library()


def run_check(cmd, lib=None, timeout=None) -> dict:
    """A check in a process of its own: its last line of output is its JSON result.  A non-zero exit fails with the tails of both outputs.
    ``lib``: the library the child loads (LAMEJS_HIP_LIB; a simulation is built first)."""
    e = dict(os.environ)
    if lib is not None:
        build_sims()
        e["LAMEJS_HIP_LIB"] = str(lib)
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, env=e, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def run_js_check(script, *args, lib=None, timeout=None) -> dict:
    """tests/<script> under node."""
    return run_check([NODE, ROOT / "tests" / script, *args], lib=lib, timeout=timeout)
