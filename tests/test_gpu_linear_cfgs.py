"""-m gpu: the forward GEMM (csrc/dvm_gemm.hip::linear_mfma_kernel) bit for bit against the C oracle under EVERY tile configuration.

tests/test_gpu_linear.py launches only what pick_cfg chooses by default (point-major 0, 4, 6 and their twins 1, 2; channel-major 0,
1); the instantiations with two row tiles per wave — point-major 3, 5, 7, channel-major 2, 3 — and configuration 0 on wide outputs
run only when DVM_LINEAR_CFG forces them.  The option is read once when the library is loaded, so each of the eight values gets a
fresh child process (tests/linear_cfg_child.py), one after another.  A child runs the case table of tests/linear_cfg_cases.py — the
point-major and channel-major tables, the row prefix, the scaled residual, `out` inside guard elements on and off the 16-byte grid,
operands off the 16-byte grid — compares every element with oracle.linear (np.array_equal: no tolerance anywhere) and every call's
dvm_linear_last_launch read-back with what the route predicates say the call must launch.  That the table reaches every edge of
every configuration is asserted without a GPU in tests/test_linear_cfg_cases_cpu.py.  The references are made once, by this process.

The parent asserts: exit status 0, the child's own "ALL COMPARED" line, the (channel_major, index, dma) triples the child saw (shown
with -s; the eight sets together are all twelve instantiations), and one SHA-256 over the point-major outputs equal in all children.

Stopping rule: a child that ends by a signal, with status 134 or 139, or at its time limit fails its test, and every later
configuration then fails at once without starting a process — nothing more goes onto a card after a fault.

CHILD_TIMEOUT: a child measured 2.0 - 2.6 s on an MI355X (the torch import and library load, then 62 GEMM launches with their
uploads and read-backs; the eight together 19 s); 60 s leaves room for a cold file cache and a busy host."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O

import linear_cfg_cases as LC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 60

_fault = []      # the configuration whose child faulted, hung or was killed: nothing is started after it
_digests = {}    # configuration -> SHA-256 of its point-major outputs


@pytest.fixture(scope="module")
def refs_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("linear_cfgs") / "refs.npz")
    np.savez(path, **LC.references(O.linear))
    return path


@pytest.mark.parametrize("c", LC.PM_CFGS)
def test_every_case_bit_exact_with_the_configuration_forced(refs_path, c):
    if _fault:
        pytest.fail("not started: the child of configuration %d faulted, hung or was killed" % _fault[0])
    code = ("import os, sys\n"
            "sys.path[:0] = [%r, os.path.join(%r, 'dv-matcher_amd'), os.path.join(%r, 'tests')]\n"
            "import linear_cfg_child\n"
            "linear_cfg_child.main(%d, %r)\n" % (ROOT, ROOT, ROOT, c, refs_path))
    env = dict(os.environ, DVM_LINEAR_CFG=str(c))
    try:
        res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _fault.append(c)
        pytest.fail("configuration %d: the child did not finish within %d s\n%s" % (c, CHILD_TIMEOUT, str(e.stderr or "")[-2000:]))
    if res.returncode < 0 or res.returncode in (134, 139):
        _fault.append(c)
    assert res.returncode == 0, "configuration %d: exit status %d\n%s" % (c, res.returncode, (res.stdout[-1000:] + res.stderr[-3000:]))
    lines = dict(ln.split(" ", 1) for ln in res.stdout.splitlines() if ln.split(" ", 1)[0] in ("TRIPLES", "DIGEST", "ALL"))
    n_refs = 2 * len(LC.PM_CASES) + len(LC.CM_CASES) + len(LC.PREFIX_CASES) + 2
    assert lines.get("ALL") == "COMPARED cfg=%d references=%d" % (c, n_refs), res.stdout[-2000:]
    triples = set(eval(lines["TRIPLES"]))
    print("DVM_LINEAR_CFG=%d launched (channel_major, index, dma): %s" % (c, sorted(triples)))
    assert triples == LC.expected_triples(c) and triples <= LC.INSTANTIATIONS
    assert (0, c, int(c >= 4)) in triples
    _digests[c] = lines["DIGEST"]
    assert len(_digests[c]) == 64 and len(set(_digests.values())) == 1, _digests
