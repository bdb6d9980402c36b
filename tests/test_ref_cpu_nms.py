"""CPU: the oracle's soft-NMS and `>=` hard-NMS restatements against the REFERENCE's own compiled Cython module
(upsnet/nms/cpu_nms.pyx, built from the reference tree into oracle/_ref by oracle/build_ref_cpu_nms.py) -- bit for bit.
This is the pin VERDICT r01 asked for: before it, soft-NMS parity rested on the oracle alone. The module's outputs are replayed
from tests/golden/ref_cpu_nms.npz (oracle/refvec.py), recorded by running this file with REFVEC_RECORD=1 where it is built."""
import os

import numpy as np
import pytest

import oracle
from conftest import ROOT, gen_dets
from oracle.refvec import RECORD, RefVectors

VEC = RefVectors(os.path.join(ROOT, "tests", "golden", "ref_cpu_nms.npz"))


class _Ref(object):
    """cpu_nms / cpu_soft_nms of the reference's module: recorded outputs, or the module itself in record mode."""

    def __init__(self):
        self.mod = oracle.ref_cpu_nms() if RECORD else None
        assert self.mod is not None or not RECORD, "oracle/_ref/upsnet_ref_cpu_nms*.so not built (make -C oracle ref)"

    def cpu_soft_nms(self, d, sigma=0.5, Nt=0.3, thr=0.001, method=0):
        want = oracle.soft_nms(d, sigma, Nt, thr, method)
        return VEC("cpu_soft_nms", (d, sigma, Nt, thr, method), want,
                   lambda: tuple(np.asarray(a) for a in self.mod.cpu_soft_nms(d.copy(), sigma, Nt, thr, method)))

    def cpu_nms(self, d, thresh):
        want = np.asarray(oracle.cpu_nms(d, thresh), np.int64)
        return VEC("cpu_nms", (d, thresh), want, lambda: np.asarray(self.mod.cpu_nms(d, thresh), np.int64))


REF = _Ref()


@pytest.fixture(scope="module", autouse=True)
def _save_records():
    yield
    VEC.save()


def _cases():
    for seed in range(4):
        for n in (1, 2, 7, 64, 65, 300, 1000):
            yield seed, n


@pytest.mark.parametrize("method", [0, 1, 2])
def test_soft_nms_equals_reference_cython(method):
    for seed, n in _cases():
        rng = np.random.default_rng(100 * method + seed)
        d = gen_dets(rng, n, ties=(seed % 2 == 0))
        for sigma, Nt, thr in ((0.5, 0.3, 0.001), (0.3, 0.5, 0.05), (0.5, 0.7, 0.3)):
            rb, ri = REF.cpu_soft_nms(d, sigma, Nt, thr, method)
            ob, oi = oracle.soft_nms(d, sigma, Nt, thr, method)
            assert np.array_equal(np.asarray(ri, np.int64), oi), (method, seed, n, Nt)
            # rows [0, N') are the result; the tail holds the reference's discarded leftovers -- compare everything
            assert np.array_equal(rb.view(np.uint32), ob.view(np.uint32)), (method, seed, n, Nt)


def test_soft_nms_empty_and_single():
    b, i = oracle.soft_nms(np.zeros((0, 5), np.float32))
    rb, ri = REF.cpu_soft_nms(np.zeros((0, 5), np.float32))
    assert b.shape == rb.shape == (0, 5) and len(i) == len(ri) == 0


@pytest.mark.parametrize("thresh", [0.3, 0.5, 0.7])
def test_cpu_nms_ge_equals_reference_cython(thresh):
    for seed, n in _cases():
        rng = np.random.default_rng(seed)
        d = gen_dets(rng, n, ties=False)
        d[:, 4] = rng.permutation(n).astype(np.float32) / n      # unique scores: numpy's argsort tie order is out of the picture
        assert list(REF.cpu_nms(d, thresh)) == oracle.cpu_nms(d, thresh), (seed, n)


def test_cpu_nms_suppresses_at_equality_and_gpu_rule_does_not():
    """cpu_nms.pyx:77 is `>=`, nms_kernel.cu:73-80 is `>`: two boxes whose IoU equals the threshold exactly."""
    a = [0, 0, 9, 9, 0.9]          # area 100
    b = [0, 5, 9, 14, 0.8]         # inter 50, union 150 -> 1/3
    d = np.array([a, b], np.float32)
    t = float(np.float32(50.0) / np.float32(150.0))   # the fp32 overlap, as a Python float
    assert list(REF.cpu_nms(d, t)) == [0] == oracle.cpu_nms(d, t)
    assert list(oracle.nms_sorted(d, t)) == [0, 1]
    # the threshold is a PYTHON float in the reference: 0.7 > float32(0.7), so an overlap of exactly float32(0.7) survives
    assert oracle.cpu_nms_sorted(d, np.nextafter(t, 1.0)).tolist() == [0, 1]
