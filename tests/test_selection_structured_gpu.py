"""GPU: the decision kernels between the RPN head and the mask head -- csrc/proposal.hip, csrc/nms.hip, csrc/detect.hip (with sort.h)
-- on the structured inputs of tests/selection_cases.py, bit for bit against the oracle: every pass of the proposal select that can
decide a cut, the greedy scan on dependency chains through whole 64-blocks and across them (all three scan forms), overlaps of
exactly the threshold, the capacity edges, the detection select at T = max_det - 1 .. 2049 with ties across the cut, the dummy ROI and
the refusals on the host; and the new NMS regimes against the reference's own `_nms` (tests/golden/ref_selection.npz, recorded as
oracle/refvec.py describes). tests/test_selection_cases_cpu.py shows that every case is in the regime it is named for."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

import oracle
from oracle import ops as oops
from oracle.refvec import RefLib, RefVectors

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import selection_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = RefVectors(os.path.join(ROOT, "tests", "golden", "ref_selection.npz"))

SPECS = {sc.case_id(s): s for s in sc.NMS_CASES + sc.PROPOSAL_CASES + sc.MASK_ROI_CASES}
NMS = [sc.case_id(s) for s in sc.NMS_CASES]
REF_NMS = [sc.case_id(s) for s in sc.REF_NMS_CASES]
EXACT = [sc.case_id(s) for s in sc.EXACT_CASES]
PROPOSALS = [sc.case_id(s) for s in sc.PROPOSAL_CASES]
MASK_ROI = [sc.case_id(s) for s in sc.MASK_ROI_CASES]
MODULE_PROPOSALS = [n for i, n in enumerate(PROPOSALS) if sc.PROPOSAL_CASES[i][0] not in [s[0] for s in sc.PROPOSAL_CASES[:i]]]


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def U():
    from upsnet_amd import ops
    return ops


@pytest.fixture(scope="module")
def ref():
    yield RefLib(VEC, os.path.join(ROOT, "oracle", "_ref", "libupsnet_ref.so"))
    VEC.save()


# inputs and oracle results are computed once per case and shared (never written to)
@functools.lru_cache(maxsize=None)
def _inputs(name):
    fn, args = SPECS[name]
    return fn(*args)[0]


@functools.lru_cache(maxsize=None)
def _nms_ref(name):
    dets, thresh = _inputs(name)
    order = oops.argsort_desc(dets[:, 4])
    sd = np.ascontiguousarray(dets[order])
    keep_sorted = oracle.nms_sorted(sd, thresh)
    keep = oops.gpu_nms(dets, thresh)
    assert np.array_equal(order[keep_sorted], keep)
    return order, sd, keep_sorted, keep


# ------------------------------------------------------------------------------------------------------------------------------ NMS
@pytest.mark.parametrize("name", NMS)
def test_nms_structured(U, name):
    """ops.gpu_nms, ops.nms_host on the sorted input and a one-problem ops.nms_batched == oracle.ops.gpu_nms / oracle.nms_sorted."""
    dets, thresh = _inputs(name)
    order, sd, keep_sorted, keep = _nms_ref(name)
    assert np.array_equal(U.gpu_nms(cu(dets), thresh).cpu().numpy(), keep)
    assert np.array_equal(U.nms_host(sd, thresh), keep_sorted)
    n = len(dets)
    k, c = U.nms_batched(cu(dets[None, :, :4]), cu(dets[None, :, 4]), cu(np.array([n], np.int32)), thresh)
    assert int(c.item()) == len(keep) and np.array_equal(k.cpu().numpy()[0, :len(keep)], keep)


@pytest.mark.parametrize("form", [0, 1, 2])
def test_nms_structured_in_every_scan_form(U, form):
    """Every case (but the 8192-box one, which the default form of test_nms_structured serves in one launch) and the batched mix
    through the three forms of the greedy scan: 0 the row-layout scan up to 1024 boxes and the general scan above, 1 the general
    scan on an LDS copy of the mask, 2 the general scan at every size."""
    from upsnet_amd._lib import lib
    try:
        lib().upsnet_nms_tuning(form)
        for name in NMS:
            dets, thresh = _inputs(name)
            if len(dets) > 2000:
                continue
            got = U.gpu_nms(cu(dets), thresh).cpu().numpy()
            assert np.array_equal(got, _nms_ref(name)[3]), (form, name)
        _check_batched_mix(U)
    finally:
        lib().upsnet_nms_tuning(0)


@functools.lru_cache(maxsize=None)
def _mix_ref():
    boxes, scores, counts, pre, thresh = sc.batched_mix()[0]
    out = []
    for p, c in enumerate(counts):
        alive = np.where(pre[p, :c] == 0)[0]
        d = np.hstack([boxes[p, :c], scores[p, :c, None]])[alive]
        out.append(alive[oops.gpu_nms(d, thresh)] if len(alive) else np.zeros((0,), np.int64))
    return out


def _check_batched_mix(U):
    boxes, scores, counts, pre, thresh = sc.batched_mix()[0]
    keep, cnt = U.nms_batched(cu(boxes), cu(scores), cu(counts), thresh, pre_removed=cu(pre))
    keep, cnt = keep.cpu().numpy(), cnt.cpu().numpy()
    for p, want in enumerate(_mix_ref()):
        assert int(cnt[p]) == len(want), p
        assert np.array_equal(keep[p, :len(want)], want), p


def test_nms_batched_mix(U):
    """One launch: a chain whose odd boxes are pre-removed, identical boxes, an empty problem, a single box, a full problem."""
    _check_batched_mix(U)


@pytest.mark.parametrize("name", EXACT)
def test_exact_threshold_through_the_ge_kernel(U, name):
    """cpu_nms_wrapper (`>=` against a double threshold) on the pairs whose overlap is the threshold: the decision is the opposite
    of the `>` kernel's on the threshold; py_nms_wrapper is the `>` rule."""
    from upsnet_amd.nms.nms import cpu_nms_wrapper, py_nms_wrapper
    dets, thresh = _inputs(name)
    order = oops.argsort_desc(dets[:, 4])
    above = float(np.nextafter(np.float32(thresh), np.float32(1)))
    for t in (thresh, above, float(np.float32(thresh)) + 1e-12):
        assert cpu_nms_wrapper(t)(dets) == oracle.cpu_nms(dets, t, order), t
    assert py_nms_wrapper(thresh)(dets) == _nms_ref(name)[3].tolist()
    assert cpu_nms_wrapper(thresh)(dets) != py_nms_wrapper(thresh)(dets) or name.endswith('below')


@pytest.mark.parametrize("name", REF_NMS)
def test_reference_nms_on_chains_ties_and_exact_thresholds(U, ref, name):
    """The reference's own `_nms` (recorded) == the oracle == ops.nms_host == ops.gpu_nms on the chain, all-same and exact-threshold
    cases. A missing record fails."""
    dets, thresh = _inputs(name)
    order, sd, want, keep = _nms_ref(name)
    n = len(sd)

    def run(lib):
        k = np.zeros((n,), np.int32)
        num = ctypes.c_int(0)
        lib.ref_nms(k.ctypes.data_as(ctypes.c_void_p), ctypes.byref(num), sd.ctypes.data_as(ctypes.c_void_p), n, 5, ctypes.c_float(thresh), 0)
        return k[:num.value]
    rk = ref("nms", (sd, thresh), want, run)
    assert np.array_equal(rk, want)
    assert np.array_equal(rk, U.nms_host(sd, thresh))
    assert np.array_equal(order[rk], U.gpu_nms(cu(dets), thresh).cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------------ proposals
@functools.lru_cache(maxsize=None)
def _prop_ref(name, individual):
    cls, box, im_info, pre, post, thr, ms = _inputs(name)
    return oops.pyramid_proposal(cls, box, im_info, pre_nms_top_n=pre, post_nms_top_n=post, nms_thresh=thr, min_size=ms,
                                 individual_proposals=individual, pad=False)


def _function(inputs, individual):
    from upsnet_amd.operators.functions.pyramid_proposal import PyramidProposalFunction
    cls, box, im_info, pre, post, thr, ms = inputs
    return PyramidProposalFunction(sc.STRIDES, (8,), (0.5, 1, 2), pre, post, thr, ms, individual_proposals=individual)


@pytest.mark.parametrize("individual", [True, False])
@pytest.mark.parametrize("name", PROPOSALS)
def test_proposals_structured(U, name, individual):
    """PyramidProposalFunction.forward_padded: kept rows, scores (as bits), the count and the zero rows past it ==
    oracle.ops.pyramid_proposal; per level, the ROI order table is a permutation with the rows past the count at its end."""
    inputs = _inputs(name)
    cls, box, im_info, pre, post, thr, ms = inputs
    ref_rois, ref_scores = _prop_ref(name, individual)
    rois, scores, num = _function(inputs, individual).forward_padded([cu(c) for c in cls], [cu(b) for b in box], cu(im_info))
    k = int(num.item())
    assert k == len(ref_scores) and k > 0
    assert tuple(rois.shape) == (post, 5) and tuple(scores.shape) == (post,)
    assert np.array_equal(bits(scores[:k].cpu().numpy()), bits(ref_scores))
    assert np.array_equal(bits(rois[:k].cpu().numpy()), bits(ref_rois))
    assert not rois[k:].any() and not scores[k:].any()
    order = getattr(rois, '_ups_roi_order', None)
    if individual and U.ROI_XCD_ORDER and U.ROI_XCD_ORDER_MIN <= post <= 2048:
        assert order is not None and order.dtype == torch.int32 and order.numel() == post
        o = order.cpu().numpy()
        assert sorted(o.tolist()) == list(range(post))
        cnt = [(post - j + 7) // 8 for j in range(8)]
        pos = np.empty(post, np.int64)
        for b in range(post):
            pos[o[b]] = sum(cnt[:b % 8]) + b // 8
        assert k == post or (pos[k:].min() >= k and pos[:k].max() < k)
    else:
        assert order is None


@pytest.mark.parametrize("name", MODULE_PROPOSALS)
def test_proposal_module_structured(U, name):
    """The PyramidProposal module, one case per builder: individual proposals, and the joint branch with its random padding drawn
    from the same generator state as the oracle's."""
    from upsnet_amd.operators.modules.pyramid_proposal import PyramidProposal
    cls, box, im_info, pre, post, thr, ms = _inputs(name)
    dc, db = [cu(c) for c in cls], [cu(b) for b in box]
    ref_rois, ref_scores = _prop_ref(name, True)
    rois, scores = PyramidProposal(sc.STRIDES, (8,), (0.5, 1, 2), pre, post, thr, ms, individual_proposals=True)(dc, db, im_info[None])
    assert np.array_equal(bits(scores.cpu().numpy()), bits(ref_scores)) and np.array_equal(bits(rois.cpu().numpy()), bits(ref_rois))
    np.random.seed(post)
    ref_rois, ref_scores = oops.pyramid_proposal(cls, box, im_info, pre_nms_top_n=pre, post_nms_top_n=post, nms_thresh=thr, min_size=ms,
                                                 individual_proposals=False)
    np.random.seed(post)
    rois, scores = PyramidProposal(sc.STRIDES, (8,), (0.5, 1, 2), pre, post, thr, ms)(dc, db, im_info[None])
    assert tuple(rois.shape) == (post, 1, 5) and tuple(scores.shape) == (post, 1, 1)
    assert np.array_equal(bits(scores.cpu().numpy().reshape(-1)), bits(ref_scores))
    assert np.array_equal(bits(rois.cpu().numpy().reshape(-1, 5)), bits(ref_rois))


# -------------------------------------------------------------------------------------------------------------------------- MaskROI
REG_WEIGHTS = (10., 10., 5., 5.)


@functools.lru_cache(maxsize=None)
def _mroi_ref(name, agn, clip, rows=None):
    rois, deltas, prob, im_info, C, st, nt, md = _inputs(name)
    r = slice(None) if rows is None else slice(0, rows)
    return oops.mask_roi(rois[r], deltas[r], prob[r], im_info, C, nt, st, md, agn, REG_WEIGHTS, clip=clip)


def _check_mask_roi(U, inputs, want, agn, clip, num_rois_dev=None):
    rois, deltas, prob, im_info, C, st, nt, md = inputs
    rs, rb, rc = want
    boxes, scores, cls, src, num = U.mask_roi(cu(rois), cu(deltas), cu(prob), cu(im_info), agn, st, nt, md, REG_WEIGHTS,
                                              num_rois_dev=num_rois_dev, clip_boxes=clip)
    n = int(num.item())
    assert n == len(rs), (n, len(rs))
    cap = boxes.shape[0]
    assert cap >= n and scores.shape[0] == cls.shape[0] == src.shape[0] == cap
    assert np.array_equal(bits(scores[:n].cpu().numpy()), bits(rs))
    assert np.array_equal(bits(boxes[:n].cpu().numpy()), bits(rb))
    assert np.array_equal(cls[:n].cpu().numpy(), rc)
    s = src[:n].cpu().numpy()
    if rc.min() >= 1:                # (not the dummy ROI) the source row of a detection holds its score
        assert (s >= 0).all() and (s < len(rois)).all() and np.array_equal(bits(prob[s, rc]), bits(rs))
    # rows past the count, up to max(max_det, MROI_FILL), are defined: zero boxes, score 0, class 0, source -1
    end = min(max(md, sc.MROI_FILL), cap)
    assert not boxes[n:end].any() and not scores[n:end].any() and not cls[n:end].any()
    assert (src[n:end] == -1).all()
    return n


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("agn", [False, True])
@pytest.mark.parametrize("name", MASK_ROI)
def test_mask_roi_structured(U, name, agn, clip):
    """ops.mask_roi: scores (as bits), boxes, classes, the count and the defined rows past it == oracle.ops.mask_roi."""
    _check_mask_roi(U, _inputs(name), _mroi_ref(name, agn, clip), agn, clip)


@pytest.mark.parametrize("agn", [False, True])
@pytest.mark.parametrize("name", ['cut-%d' % (sc.MAX_DET + 1), 'cut_in_tie', 'nothing_above_threshold', 'sparse_classes-81'])
def test_mask_roi_module_structured(U, name, agn):
    """The MaskROI module (max_det from the configuration)."""
    from upsnet_amd.config.config import config
    from upsnet_amd.operators.modules.mask_roi import MaskROI
    rois, deltas, prob, im_info, C, st, nt, md = _inputs(name)
    saved = config.dataset.num_classes, config.test.max_det
    try:
        config.dataset.num_classes, config.test.max_det = C, md
        for clip in (True, False):
            rs, rb, rc = _mroi_ref(name, agn, clip)
            s, b, c = MaskROI(clip, False, md, C, nms_thresh=nt, class_agnostic=agn, score_thresh=st)(cu(rois), cu(deltas), cu(prob), im_info)
            assert np.array_equal(bits(s.cpu().numpy()), bits(rs)) and np.array_equal(bits(b.cpu().numpy()), bits(rb))
            assert np.array_equal(c.cpu().numpy(), rc)
    finally:
        config.dataset.num_classes, config.test.max_det = saved


SPECS[sc.case_id((sc.device_count, []))] = (sc.device_count, [])


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("agn", [False, True])
def test_mask_roi_device_count(U, agn, clip):
    """A device-side count below the capacity: the result is the oracle's on the valid rows, whatever the others hold."""
    name = sc.case_id((sc.device_count, []))
    n, cap = sc.DEVICE_COUNT
    dev = torch.tensor([n], dtype=torch.int32, device='cuda')
    _check_mask_roi(U, _inputs(name), _mroi_ref(name, agn, clip, n), agn, clip, num_rois_dev=dev)
    # a count above the capacity is clamped to it
    dev = torch.tensor([cap + 1000], dtype=torch.int32, device='cuda')
    _check_mask_roi(U, _inputs(name), _mroi_ref(name, agn, clip), agn, clip, num_rois_dev=dev)


# ------------------------------------------------------------------------------------------------------------------ host refusals
def test_capacity_limits_are_refused_on_the_host(U):
    """8193 boxes per problem are refused before anything is launched (8192 is served: none_overlap-8192); more than 8192
    class-agnostic candidates above the score threshold come back as a negative count, which the module turns into an error."""
    from upsnet_amd.config.config import config
    from upsnet_amd.operators.modules.mask_roi import MaskROI, check_count
    d = sc.none_overlap(8192)[0][0]
    d = np.vstack([d, d[:1] + np.float32([0, 2000, 0, 2000, 0])])
    with pytest.raises(RuntimeError, match="8192"):
        U.nms_host(d, 0.5)
    with pytest.raises(RuntimeError, match="8192"):
        U.nms_batched(cu(d[None, :, :4]), cu(d[None, :, 4]), cu(np.array([8193], np.int32)), 0.5)
    with pytest.raises(RuntimeError, match="8192"):
        U.gpu_nms(cu(d), 0.5)
    rois, deltas, prob, im_info, C, st, nt, md = sc.agnostic_overflow()[0]
    boxes, scores, cls, src, num = U.mask_roi(cu(rois), cu(deltas), cu(prob), cu(im_info), True, st, nt, md, REG_WEIGHTS)
    assert int(num.item()) < 0
    with pytest.raises(RuntimeError, match="8192"):
        check_count(int(num.item()))
    saved = config.dataset.num_classes, config.test.max_det
    try:
        config.dataset.num_classes, config.test.max_det = C, md
        with pytest.raises(RuntimeError, match="8192"):
            MaskROI(True, False, md, C, nms_thresh=nt, class_agnostic=True, score_thresh=st)(cu(rois), cu(deltas), cu(prob), im_info)
        # class-wise the same input is an ordinary case of 1030 candidates per class
        s, b, c = MaskROI(True, False, md, C, nms_thresh=nt, class_agnostic=False, score_thresh=st)(cu(rois), cu(deltas), cu(prob), im_info)
        assert len(s) >= md
    finally:
        config.dataset.num_classes, config.test.max_det = saved
    torch.cuda.synchronize()
