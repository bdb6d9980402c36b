"""CPU: the judge of the GPU suite -- oracle/c/upsnet_oracle.c -- under AddressSanitizer and UndefinedBehaviorSanitizer.

Code loaded into Python cannot run under a sanitizer, so every C call the wrappers of oracle/__init__.py make is recorded
(oracle/replay.py) and replayed in oracle/c/orc_replay.c, a program of its own that allocates every buffer at exactly its documented
size. The inputs are the edge rows of the GPU tests (tests/test_ops_gpu.py, test_backward_gpu.py, test_preprocess_gpu.py,
panoptic_cases.py, selection_cases.py) at their smallest parametrisation, plus coordinates of 1e9, 3e38, +-inf and NaN. For every
recorded call:
  1. the sanitized -O1 driver exits 0 with an empty stderr;
  2. the sanitized -O1 driver, the plain -O2 driver and the ctypes library give the same bits;
  3. the outputs do not depend on what the output buffers held before the call (fill bytes 0x00 and 0xA5);
  4. the outputs do not depend on orc_set_threads (1 and 4).
No GPU, no LD_PRELOAD: the children run with HIP_VISIBLE_DEVICES and ROCR_VISIBLE_DEVICES empty.
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import oracle.ops as oops
from oracle import replay

import panoptic_cases as PC
import selection_cases as SC
from conftest import gen_dets, gen_rois

pytestmark = pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc is not installed: the sanitized replay driver cannot be built")

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
MEANS = np.array((102.9801, 115.9465, 122.7717,))

# The part of each output that the function's contract defines, where that is not the whole buffer. (outputs, ret) -> outputs.
#   orc_nms_sorted / orc_cpu_nms_sorted   "Returns the number kept; keep_out[] = indices into the SORTED array in visiting order":
#                                         entries past the returned count are not written.
#   orc_mask_removal                      "Outputs keep_inds (original indices, visiting order) and ... the pasted logits [k, H, W]":
#                                         k is the return value; rows of keep_inds and planes of mask_energy past k are not written.
#                                         The occupancy scratch is "zeroed here": all of it is defined.
DEFINED = {
    "orc_nms_sorted": lambda outs, ret: [outs[0][:ret]],
    "orc_cpu_nms_sorted": lambda outs, ret: [outs[0][:ret]],
    "orc_mask_removal": lambda outs, ret: [outs[0], outs[1][:ret]] + [o[:ret] for o in outs[2:]],
}


# ------------------------------------------------------------------------------------------------------------------------ inputs
def extreme_rows():
    """Boxes a detector head can emit when its logits blow up: (x1, y1, x2, y2)."""
    big, huge = F32(1e9), F32(3e38)
    return np.array([[-big, -big, big, big], [big, big, big + 64, big + 64], [-huge, -huge, huge, huge], [huge, 0, huge, 9],
                     [-INF, -INF, INF, INF], [INF, INF, INF, INF], [-INF, 2, -INF, 9], [NAN, 3, 20, 9], [2, NAN, 9, NAN],
                     [NAN, NAN, NAN, NAN], [3, 2, INF, 9], [3, 2, 9, NAN]], F32)


def roi_rows(H, W, scale, batch=1):
    """tests/test_ops_gpu.py::test_roi_align_nchw_bitexact and test_backward_gpu.py::test_roi_align_backward: random ROIs, then
    degenerate, wholly outside (both sides), inverted, partly outside; batch index 1 on every third row when there are two images."""
    rng = np.random.default_rng(0)
    rois = gen_rois(rng, 12, int(H / scale), int(W / scale), 4, max(8, int(H / scale)))
    if batch > 1:
        rois[::3, 0] = 1
    edge = [[0, 0, 0, 0, 0], [batch - 1, -20, -20, -5, -5], [0, W / scale + 50, 3, W / scale + 90, 9], [0, 10, 10, 5, 5],
            [0, -40, -30, 20, 25], [0, W / scale - 10, H / scale - 12, W / scale + 60, H / scale + 40], [0, 17.3, 21.9, 17.3, 21.9],
            [batch - 1, -300, -300, -200, -250]]
    return np.vstack([rois, edge]).astype(F32)


def with_extremes(rois5):
    ex = extreme_rows()
    return np.vstack([rois5, np.hstack([np.zeros((len(ex), 1), F32), ex])]).astype(F32)


def case_roi_align():
    for (C, H, W, ph, scale, sr, batch) in [(4, 5, 7, 7, 1.0 / 32, 2, 1), (3, 1, 1, 2, 0.25, 2, 1), (2, 5, 7, 3, 0.25, 0, 2),
                                            (2, 20, 30, 7, 0.25, 2, 2)]:
        rng = np.random.default_rng(C + H)
        feat = rng.normal(size=(batch, C, H, W)).astype(F32)
        rois = roi_rows(H, W, scale, batch)
        rois = with_extremes(rois)     # (sampling_ratio 0: the oracle refuses a ROI whose adaptive grid passes ORC_MAX_GRID)
        oracle.roi_align_forward(feat, rois, ph, ph, scale, sr)
        top = rng.normal(size=(rois.shape[0], C, ph, ph)).astype(F32)
        oracle.roi_align_backward(top, rois, (batch, C, H, W), scale, sr)


def _dcn_inputs(rng, B, C, H, W, k, pad, stride, dil, dg):
    Ho, Wo = oracle._col_geom(H, W, (k, k), pad, (stride, stride), (dil, dil))
    im = rng.normal(size=(B, C, H, W)).astype(F32)
    off = (rng.normal(size=(B, dg * 2 * k * k, Ho, Wo)) * 2.5).astype(F32)
    mask = rng.uniform(0, 2, size=(B, dg * k * k, Ho, Wo)).astype(F32)
    col = rng.normal(size=(C * k * k, B, Ho, Wo)).astype(F32)
    # test_ops_gpu.py::test_deform_im2col_bitexact and test_backward_gpu.py::test_deform_col2im_coord_bit_exact
    off[:, :, 0, 0] = 0.0
    if Ho > 1 and Wo > 1:
        off[:, 0, 1, 1] = -1.0 - pad[0]                        # lands exactly on the -1 border
    off[:, 0, 0, :] = -40.0
    off[:, 1, min(1, Ho - 1), :] = 200.0
    off[:, 2, min(2, Ho - 1), :] = F32(-1.0) - (np.arange(Wo) % 2)
    return im, off, mask, col


def _dcn_extremes(off):
    """1e9, 3e38, +-inf and NaN in both offset channels of the last tap, at the first pixels of the last row."""
    vals = [F32(1e9), F32(-1e9), F32(3e38), F32(-3e38), INF, -INF, NAN]
    off = off.copy()
    flat = off.reshape(off.shape[0], off.shape[1], -1)
    for i, v in enumerate(vals):
        p = flat.shape[2] - 1 - i
        if p < 0:
            break
        flat[:, -1 - (i % 2), p] = v
        if i >= 4:
            flat[:, -2 + (i % 2), p] = v
    return off


def case_deform():
    # (C, H, W, k, pad, stride, dil, dg): the geometries of test_ops_gpu.py / test_backward_gpu.py CASES at their smallest, stride 2,
    # dilation 2 with two deformable groups, pad_h != pad_w (test_mod_col2im_pad_quirk), a 1 x 1 map
    for (C, H, W, k, pad, stride, dil, dg) in [(4, 6, 7, 3, (1, 1), 1, 1, 1), (4, 9, 9, 3, (2, 2), 1, 2, 2), (2, 8, 8, 3, (1, 1), 2, 1, 1),
                                               (2, 6, 7, 3, (1, 2), 1, 1, 1), (2, 1, 1, 3, (1, 1), 1, 1, 2)]:
        rng = np.random.default_rng(3 + H)
        im, off, mask, col = _dcn_inputs(rng, 2, C, H, W, k, pad, stride, dil, dg)
        args = ((k, k), pad, (stride, stride), (dil, dil))
        for o in (off, _dcn_extremes(off)):
            for m in (None, mask):
                oracle.deform_im2col(im[1], o[1], *args, dg, mask=None if m is None else m[1])
                oracle.deform_col2im(col, o, im.shape, *args, dg, mask=m)
                oracle.deform_col2im_coord(col, im, o, *args, dg, mask=m)


def _sorted(d):
    return d[oops.argsort_desc(d[:, 4])]


def case_nms():
    rng = np.random.default_rng(1)
    sets = [(gen_dets(rng, 1), 0.5), (gen_dets(rng, 65), 0.5), (gen_dets(rng, 65), 0.7), SC.degenerate()[0], SC.all_same(65, True)[0],
            SC.exact_threshold(0.5, 'exact')[0], SC.exact_threshold(0.7, 'below')[0], SC.chain(65, 0.7, True)[0]]
    ex = extreme_rows()
    sets.append((np.hstack([ex, np.linspace(0.9, 0.1, len(ex), dtype=F32)[:, None]]), 0.5))
    nan_score = gen_dets(rng, 9)
    nan_score[3, 4], nan_score[5, 4] = NAN, INF
    sets.append((nan_score, 0.5))
    for d, t in sets:
        d = np.asarray(d, F32)
        oracle.nms_sorted(_sorted(d), t)
        oracle.cpu_nms_sorted(_sorted(d), t)
        oracle.nms_sorted(_sorted(d)[:, :4], t)                 # box_dim 4: the stride of the rows is an argument
        for method in (0, 1, 2):
            oracle.soft_nms(d, 0.5, 0.3, 0.001 if method else 0.05, method)
    # n = 0: the wrappers answer themselves (no C call); the pair of test_cpu_nms_ge_bitexact whose overlap is the threshold
    assert len(oracle.nms_sorted(np.zeros((0, 5), F32), 0.5)) == 0 and oracle.cpu_nms(np.zeros((0, 5), F32), 0.5) == []
    assert len(oracle.soft_nms(np.zeros((0, 5), F32))[1]) == 0
    a = np.array([[0, 0, 9, 9, 0.9], [0, 5, 9, 14, 0.8]], F32)
    t = float(F32(50.0) / F32(150.0))
    assert list(oracle.cpu_nms_sorted(a, t)) == [0] and list(oracle.nms_sorted(a, t)) == [0, 1]
    assert list(oracle.cpu_nms_sorted(a, float(np.nextafter(t, 1.0)))) == [0, 1]


def _head(case, void=True):
    fcn, rois5, prob, logit, cls, S, C, H, W = case
    return oops.panoptic_head(fcn, rois5, prob, logit, cls, S, C, enable_void=void)


def case_panoptic():
    # m = 1; fractional corners clipped at 0, a box over the whole image, boxes narrower than a pixel, inverted and outside boxes
    # (panoptic_cases.word_edges); the overlap ratio of exactly 3/10; S = 133 / C = 81; a 1 x 1 map
    rng = np.random.default_rng(20)
    one = PC._pack(rng, *PC._random(rng, 1, 9, 16, 16), 9, 16, 16, S=19)
    for void in (True, False):
        _head(one, void)
        _head(PC.word_edges(65)[0], void)
    for v in ('exact', 'plus', 'minus'):
        _head(PC.threshold_exact(v)[0])
    rng = np.random.default_rng(302)
    _head(PC._pack(rng, *PC._random(rng, 8, 9, 24, 32, ms=2), 9, 24, 32, S=19))       # panoptic_cases.mask_side(2) on a smaller map
    _head(PC.exact_ties()[0], False)
    rng = np.random.default_rng(133)
    _head(PC._pack(rng, *PC._random(rng, 12, 81, 12, 13), 81, 12, 13, S=133))
    rng = np.random.default_rng(11)
    _head(PC._pack(rng, [[0, 0, 0, 0], [-0.5, -0.5, 0.5, 0.5]], [0.9, 0.8], PC._const_logit(2), [1, 2], 3, 1, 1))
    # nothing kept (all logits negative), energy not wanted
    fcn, rois5, prob, logit, cls, S, C, H, W = PC.mask_side(14)[0]
    oops.mask_removal(rois5[:, 1:], prob, -np.abs(logit) - 1, cls, (H, W), want_energy=False)
    # extreme boxes through the removal and, scaled as SegTerm scales them, through the seg term
    ex = extreme_rows()
    m = len(ex)
    rng = np.random.default_rng(m)
    fcn = rng.normal(0, 3, size=(1, 12, 9, 11)).astype(F32)
    cls = (1 + np.arange(m) % 8).astype(np.int64)
    oops.mask_removal(ex, np.linspace(0.9, 0.5, m, dtype=F32), PC._const_logit(m), cls, (9, 11))
    oops.seg_term(cls, fcn, np.hstack([np.zeros((m, 1), F32), ex]), 12, 9)
    oops.seg_term(np.zeros(2, np.int64), fcn, np.zeros((2, 5), F32), 12, 9)          # class 0: the plane stays zero


def case_resize_upsample_prep():
    rng = np.random.default_rng(5)
    src = rng.normal(size=(28, 28)).astype(F32)
    for dw, dh in [(1, 1), (28, 28), (3, 70), (57, 5)]:
        oracle.resize_bilinear(src, dw, dh)
    oracle.resize_bilinear(src[:1, :1], 5, 3)
    oracle.resize_bilinear(src[:2, :2], 1, 7)
    for dx, dy in [(0, 0), (4, 2), (56, 4)]:
        oracle.lib().orc_resize_at(oracle._p(src), 28, 57, 5, dx, dy)
    for Hs, Ws, S in PC.UP_TINY[:2] + [(3, 7, 19)]:
        score = rng.normal(0, 3, size=(S, Hs, Ws)).astype(F32)
        oracle.upsample_bilinear(score, 4)
        oracle.upsample_bilinear(score, 1)
    for H, W, S, nlev, bias in [(1, 1, 3, 1, True), (8, 8, 5, 4, True), (8, 24, 19, 3, False), (4, 12, 2, 2, True)]:
        parts = [rng.normal(size=(H >> l, W >> l, S)).astype(F32) for l in range(nlev)]
        oracle.fcn_score_combine(parts, rng.normal(size=S).astype(F32) if bias else None)
    # tests/test_preprocess_gpu.py: identity, down- and up-scaling at odd sizes; a 1 x 1 image
    for H, W, target, max_size in [(16, 32, 16, 32), (25, 37, 25, 50), (24, 40, 20, 30), (19, 27, 32, 48), (30, 23, 15, 1000), (1, 1, 1, 1),
                                   (1, 1, 3, 8)]:
        im = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        oracle.prep_image(im, MEANS, target, max_size)


def case_set_threads():
    oracle.set_threads(3)
    oracle.set_threads(0)
    oracle.set_threads(1)


CASES = [case_roi_align, case_deform, case_nms, case_panoptic, case_resize_upsample_prep, case_set_threads]
MAX_INPUT_BYTES = 320 << 10     # cases stay tiny: tens of kilobytes, the fuse of panoptic_cases.word_edges(65) (taken as it is) 270 KiB


@functools.lru_cache(maxsize=None)
def recorded(fn):
    oracle.set_threads(1)
    with replay.recording() as calls:
        fn()
    return tuple(calls)


# ------------------------------------------------------------------------------------------------------------------------- tests
def exported_orc_symbols():
    out = subprocess.check_output(["nm", "-D", "--defined-only", oracle.build()]).decode()
    return sorted(line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("orc_"))


def test_every_exported_function_has_a_case():
    """A function added to upsnet_oracle.c without a case here (and without an entry in oracle/replay.py and orc_replay.c) fails."""
    driven = sorted({c.name for fn in CASES for c in recorded(fn)})
    exported = exported_orc_symbols()
    assert len(exported) >= 17
    assert driven == exported, "exported but not driven: %s; driven but not exported: %s" % (
        sorted(set(exported) - set(driven)), sorted(set(driven) - set(exported)))
    assert sorted(replay.FUNCS) == exported


STRICT = [True]     # set per recorded call by the test below


def ordinary_inputs(case):
    """True when every floating-point input of the call is finite and below 1e8 in magnitude: every case but the extreme rows."""
    return all(np.isfinite(a).all() and (np.abs(a) < 1e8).all() for role, a in case.records
               if role in (replay.IN, replay.INOUT) and np.asarray(a).dtype.kind == 'f')


def _bits(x):
    """The array's bytes. For a call with ordinary inputs that is all: the comparison is bitwise. For a call that carries the
    extreme rows (1e9, 3e38, inf, NaN) every NaN is first replaced by the one canonical quiet NaN: IEEE 754 leaves the sign and
    payload of a NaN RESULT open (x86 gives inf - inf and 0 * inf the sign bit, a folded constant or a negation moved by the
    optimiser does not), so they are no property of the C source. Where a NaN stands, and every bit of every other value, must agree."""
    if x.dtype.kind == 'f' and not STRICT[0]:
        x = np.where(np.isnan(x), x.dtype.type(np.nan), x)
    return np.ascontiguousarray(x).tobytes()


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and _bits(x) == _bits(y) for x, y in zip(a, b))


def _ret_same(a, b):
    return _bits(np.asarray(a, np.float32)) == _bits(np.asarray(b, np.float32)) if isinstance(a, float) else a == b


@pytest.mark.parametrize("fn", CASES, ids=lambda f: f.__name__)
def test_replay_is_clean_and_bit_stable(fn):
    san, o2 = oracle.build_replay(sanitize=True), oracle.build_replay(sanitize=False)
    calls = recorded(fn)
    assert calls
    for n, case in enumerate(calls):
        tag = "%s call %d (%s)" % (fn.__name__, n, case.name)
        assert case.input_bytes() <= MAX_INPUT_BYTES, tag
        region = DEFINED.get(case.name, lambda outs, ret: outs)
        STRICT[0] = ordinary_inputs(case)
        # 1. clean under ASan + UBSan
        ret_a, out_a, report = replay.run(san, case, fill=0x00, threads=1)
        assert report == "", "%s: the sanitized driver reported\n%s" % (tag, report)
        # 2. sanitized -O1 == plain -O2 == ctypes, on the defined region (and the return value)
        ret_b, out_b, report = replay.run(o2, case, fill=0x00, threads=1)
        assert report == "", "%s: the -O2 driver reported\n%s" % (tag, report)
        assert _ret_same(ret_a, ret_b) and _ret_same(ret_a, case.ret if case.ret is not None else 0), (tag, ret_a, ret_b, case.ret)
        want = region(case.outputs, case.ret)
        assert _same(region(out_a, ret_a), want), "%s: sanitized -O1 driver and ctypes library differ" % tag
        assert _same(region(out_b, ret_b), want), "%s: -O2 driver and ctypes library differ" % tag
        # 3. nothing of the defined region is left as the buffer was
        ret_c, out_c, report = replay.run(san, case, fill=0xA5, threads=1)
        assert report == "", "%s: the sanitized driver reported (fill 0xA5)\n%s" % (tag, report)
        assert _ret_same(ret_a, ret_c) and _same(region(out_c, ret_c), want), "%s: output depends on the buffer's previous contents" % tag
        # 4. nor on the thread count
        ret_d, out_d, report = replay.run(o2, case, fill=0xA5, threads=4)
        assert report == "", "%s: the -O2 driver reported (4 threads)\n%s" % (tag, report)
        assert _ret_same(ret_a, ret_d) and _same(region(out_d, ret_d), want), "%s: output depends on orc_set_threads" % tag

