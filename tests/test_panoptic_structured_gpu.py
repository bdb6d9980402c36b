"""GPU: the panoptic head kernels (upsnet_amd/csrc/panoptic.hip) on the structured inputs of tests/panoptic_cases.py, bit for bit
against the oracle: the candidate-overflow path and the chains of removal rounds of mask_removal_kernel, its sort path for more than
256 instances and its tables at 1024, the decision at exactly 3/10, score ties, mask sides 2 / 14 / 32, boxes on the bitmap word
edges, a device-side count; the scalar-load form panoptic_fuse_kernel<1> (widths that are no multiple of 4, a pointer that is not
16-byte aligned), 256 kept instances, exact argmax ties, the fused-upsample kernel on tiny maps and with 160 classes; and the
capacity checks of the entry points. tests/test_panoptic_cases_cpu.py shows that every case is in the regime it is named for."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import oracle
from oracle import ops as oops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import panoptic_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

SPECS = {pc.case_id(s): s for s in pc.REMOVAL_CASES}
REMOVAL = [pc.case_id(s) for s in pc.REMOVAL_CASES]
FUSE = [pc.case_id(s) for s in pc.FUSE_CASES]


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


@pytest.fixture(scope="module")
def U():
    from upsnet_amd import ops
    return ops


# inputs and oracle results are computed once per case and shared (never written to)
@functools.lru_cache(maxsize=None)
def _inputs(name):
    fn, args = SPECS[name]
    return fn(*args)[0]


@functools.lru_cache(maxsize=None)
def _keep_ref(name):
    fcn, rois5, prob, logit, cls, S, C, H, W = _inputs(name)
    return oops.mask_removal(rois5[:, 1:], prob, logit, cls, (H, W), want_energy=False)[0]


@functools.lru_cache(maxsize=None)
def _head_ref(name, void):
    fcn, rois5, prob, logit, cls, S, C, H, W = _inputs(name)
    return oops.panoptic_head(fcn, rois5, prob, logit, cls, S, C, enable_void=void)


@functools.lru_cache(maxsize=None)
def _up_ref(name):
    """A seeded low-resolution score, its x4 upsampling (the oracle's) and the head on it (the setup of
    test_ops_gpu.test_panoptic_fuse_with_fused_upsample_bitexact)."""
    _, rois5, prob, logit, cls, S, C, H, W = _inputs(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    score = rng.normal(0, 3, size=(1, S, H // 4, W // 4)).astype(np.float32)
    fcn = oracle.upsample_bilinear(score[0], 4)[None]
    return score, oops.panoptic_head(fcn, rois5, prob, logit, cls, S, C, enable_void=True)


def _removal(U, inputs, m_dev=None):
    fcn, rois5, prob, logit, cls, S, C, H, W = inputs
    return U.mask_removal(cu(rois5[:, 1:]), cu(prob), cu(logit), cu(cls), C - 1, (H, W), m_dev=m_dev)


def _check_keep(keep, num, real, ref_keep, ref_real=1):
    k = int(num.item())
    got = keep.cpu().numpy()
    assert k == len(ref_keep), (k, len(ref_keep))
    assert np.array_equal(got[:k], ref_keep)
    assert int(real.item()) == ref_real
    assert not got[k:].any(), "keep rows past the count are not 0"
    return k


@pytest.mark.parametrize("name", REMOVAL)
def test_mask_removal_structured(U, name):
    """Keep list, count, real_keep and the zero rows past the count == oracle.ops.mask_removal."""
    inputs = _inputs(name)
    keep, num, real = _removal(U, inputs)
    ref = _keep_ref(name)
    # (every case keeps something: the oracle's [0] of the empty branch never stands for 'nothing kept' here)
    _check_keep(keep, num, real, ref)


def test_mask_removal_nothing_kept_at_capacity(U):
    """1024 instances of one class, every logit negative: the fallback keep = [0], real_keep = 0."""
    fcn, rois5, prob, logit, cls, S, C, H, W = _inputs('many-1024-True')
    neg = -np.abs(logit) - np.float32(1)
    ref, _ = oops.mask_removal(rois5[:, 1:], prob, neg, cls, (H, W), want_energy=False)
    assert ref.tolist() == [0]
    keep, num, real = U.mask_removal(cu(rois5[:, 1:]), cu(prob), cu(neg), cu(cls), C - 1, (H, W))
    _check_keep(keep, num, real, ref, ref_real=0)


def test_mask_removal_device_count(U):
    """Capacity 64, 37 valid rows by a device-side count: the result is the oracle's on the first 37 rows, whatever the others hold."""
    (fcn, rois5, prob, logit, cls, S, C, H, W), _ = pc.device_count()
    n = pc.DEVICE_COUNT
    ref, _ = oops.mask_removal(rois5[:n, 1:], prob[:n], logit[:n], cls[:n], (H, W), want_energy=False)
    m_dev = torch.tensor([n], dtype=torch.int32, device='cuda')
    keep, num, real = _removal(U, (fcn, rois5, prob, logit, cls, S, C, H, W), m_dev=m_dev)
    assert keep.shape[0] == 64
    _check_keep(keep, num, real, ref)
    # a count above the capacity is clamped to it
    name = 'mask_side-14'
    keep, num, real = _removal(U, _inputs(name), m_dev=torch.tensor([1000], dtype=torch.int32, device='cuda'))
    _check_keep(keep, num, real, _keep_ref(name))


def _fuse_args(inputs):
    fcn, rois5, prob, logit, cls, S, C, H, W = inputs
    return S - (C - 1), cu(rois5), cu(logit), cu(cls), cu(oops.class_mapping(S, C))


@pytest.mark.parametrize("void", [True, False])
@pytest.mark.parametrize("name", FUSE)
def test_panoptic_fuse_structured(U, name, void):
    """ops.mask_removal -> ops.panoptic_fuse, and -> mask_paste + seg_term + panoptic_argmax: semantic and panoptic maps ==
    oracle.ops.panoptic_head. Where the width is no multiple of 4 the fused kernel runs in its scalar-load form (the dispatch of
    upsnet_panoptic_fuse has no other); its map is then also compared with the float4 form's on a width-padded copy."""
    inputs = _inputs(name)
    fcn, rois5, prob, logit, cls, S, C, H, W = inputs
    ref = _head_ref(name, void)
    keep, num, real = _removal(U, inputs)
    k = _check_keep(keep, num, real, ref['keep_inds'])
    s_stuff, r5, lg, ci, cmap = _fuse_args(inputs)
    f = cu(fcn)
    assert f.data_ptr() % 16 == 0
    pan, sem = U.panoptic_fuse(f, s_stuff, r5, lg, ci, keep, num, real, cmap, void)
    assert np.array_equal(sem.cpu().numpy()[0], ref['sem'])
    assert np.array_equal(pan.cpu().numpy()[0], ref['panoptic'])
    energy = U.mask_paste(r5[:, 1:], lg, keep, num, real, k, (H, W))
    kk = keep[:k]
    seg_inst = U.seg_term(f, (r5[kk] * 4.0)[:, 1:] * 0.25, ci[kk], cmap)
    pan2 = U.panoptic_argmax(f, s_stuff, seg_inst, energy, void)
    assert np.array_equal(pan2.cpu().numpy()[0], ref['panoptic'])
    if W % 4 != 0 and float(rois5[:, 1:].min()) >= 0:     # (a negative coordinate is a Python slice index counted from W)
        Wp = (W + 3) // 4 * 4
        fp = torch.zeros((1, S, H, Wp), dtype=torch.float32, device='cuda')
        fp[..., :W] = f
        assert fp.data_ptr() % 16 == 0
        pan4, sem4 = U.panoptic_fuse(fp, s_stuff, r5, lg, ci, keep, num, real, cmap, void)
        assert torch.equal(pan4[..., :W], pan) and torch.equal(sem4[..., :W], sem)


@pytest.mark.parametrize("void", [True, False])
def test_panoptic_fuse_misaligned_pointer(U, void):
    """fcn_output one float into a larger buffer (W % 4 == 0, pointer % 16 == 4): a read-only input, so the wrapper hands the kernel an
    aligned copy (the kernel's scalar-load form for such a base is no longer reached from Python); same bits as the
    aligned call and the oracle."""
    from upsnet_amd._lib import f32c
    inputs = _inputs('misaligned')
    fcn, rois5, prob, logit, cls, S, C, H, W = inputs
    assert W % 4 == 0
    ref = _head_ref('misaligned', void)
    keep, num, real = _removal(U, inputs)
    s_stuff, r5, lg, ci, cmap = _fuse_args(inputs)
    aligned = cu(fcn)
    buf = torch.empty(aligned.numel() + 4, dtype=torch.float32, device='cuda')
    view = buf[1:1 + aligned.numel()].view(aligned.shape)
    view.copy_(aligned)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    assert f32c(view).data_ptr() % 16 == 0 and torch.equal(f32c(view), view) and f32c(aligned) is aligned
    pan_a, sem_a = U.panoptic_fuse(aligned, s_stuff, r5, lg, ci, keep, num, real, cmap, void)
    pan_m, sem_m = U.panoptic_fuse(view, s_stuff, r5, lg, ci, keep, num, real, cmap, void)
    assert np.array_equal(pan_m.cpu().numpy()[0], ref['panoptic']) and np.array_equal(sem_m.cpu().numpy()[0], ref['sem'])
    assert torch.equal(pan_m, pan_a) and torch.equal(sem_m, sem_a)


UP = [n for n in FUSE if _inputs(n)[7] % 4 == 0 and _inputs(n)[8] % 4 == 0]


@pytest.mark.parametrize("nhwc", [True, False])
@pytest.mark.parametrize("name", UP)
def test_panoptic_fuse_up_structured(U, name, nhwc):
    """ops.panoptic_fuse_up on a low-resolution score == the oracle's head on the oracle's x4 upsampling of it."""
    inputs = _inputs(name)
    score, ref = _up_ref(name)
    keep, num, real = _removal(U, inputs)
    _check_keep(keep, num, real, ref['keep_inds'])
    s_stuff, r5, lg, ci, cmap = _fuse_args(inputs)
    sc = cu(score)
    if nhwc:
        sc = sc.contiguous(memory_format=torch.channels_last)
    pan, sem = U.panoptic_fuse_up(sc, 4, s_stuff, r5, lg, ci, keep, num, real, cmap)
    assert np.array_equal(sem.cpu().numpy()[0], ref['sem'])
    assert np.array_equal(pan.cpu().numpy()[0], ref['panoptic'])


@pytest.mark.parametrize("nhwc", [True, False])
@pytest.mark.parametrize("Hs,Ws,S", pc.UP_TINY)
def test_panoptic_fuse_up_tiny(U, Hs, Ws, S, nhwc):
    """Score maps smaller than the kernel's source patch (1 x 1, 2 x 3, 3 x 70), and 160 semantic classes."""
    (score, rois5, prob, logit, cls, S_, C, H, W), _ = pc.up_tiny(Hs, Ws, S)
    fcn = oracle.upsample_bilinear(score[0], 4)[None]
    ref = oops.panoptic_head(fcn, rois5, prob, logit, cls, S, C, enable_void=True)
    inputs = (fcn, rois5, prob, logit, cls, S, C, H, W)
    keep, num, real = _removal(U, inputs)
    _check_keep(keep, num, real, ref['keep_inds'])
    s_stuff, r5, lg, ci, cmap = _fuse_args(inputs)
    sc = cu(score)
    if nhwc:
        sc = sc.contiguous(memory_format=torch.channels_last)
    pan, sem = U.panoptic_fuse_up(sc, 4, s_stuff, r5, lg, ci, keep, num, real, cmap)
    assert np.array_equal(sem.cpu().numpy()[0], ref['sem'])
    assert np.array_equal(pan.cpu().numpy()[0], ref['panoptic'])
    pan1, sem1 = U.panoptic_fuse(cu(fcn), s_stuff, r5, lg, ci, keep, num, real, cmap, True)
    assert torch.equal(pan1, pan) and torch.equal(sem1, sem)


# ------------------------------------------------------------------------------------------------------------------ capacity edges
# Every limit is checked on the host before anything is launched: upsnet_mask_removal, upsnet_panoptic_fuse and upsnet_panoptic_fuse_up
# open with their UPS_REQUIREs, and the Python wrappers of the fused kernels refuse more than 256 rows themselves.
def _small(m, ms=28, S=19, C=9, H=32, W=48):
    rng = np.random.default_rng(m + ms)
    rois = np.zeros((m, 5), np.float32)
    rois[:, 1:] = [2, 3, 20, 17]
    return (rng.normal(0, 1, (1, S, H, W)).astype(np.float32), rois, np.linspace(0.9, 0.5, m).astype(np.float32),
            np.ones((m, 1, ms, ms), np.float32), np.ones(m, np.int64), S, C, H, W)


def _kept_one():
    return (torch.zeros(1, dtype=torch.int64, device='cuda'), torch.ones(1, dtype=torch.int32, device='cuda'),
            torch.ones(1, dtype=torch.int32, device='cuda'))


def test_capacity_limits_are_refused_on_the_host(U):
    with pytest.raises(RuntimeError, match="1024"):
        _removal(U, _small(1025))
    keep, num, real = _removal(U, _small(1024))
    assert int(num.item()) == 1 and int(real.item()) == 1        # (1024 itself is served: identical boxes, the first is kept)
    for m, ok in [(256, True), (257, False)]:
        inputs = _small(m)
        s_stuff, r5, lg, ci, cmap = _fuse_args(inputs)
        sc = torch.zeros((1, 19, 8, 12), device='cuda')
        if ok:
            U.panoptic_fuse(cu(inputs[0]), s_stuff, r5, lg, ci, *_kept_one(), cmap, True)
            U.panoptic_fuse_up(sc, 4, s_stuff, r5, lg, ci, *_kept_one(), cmap)
        else:
            with pytest.raises(RuntimeError, match="256"):
                U.panoptic_fuse(cu(inputs[0]), s_stuff, r5, lg, ci, *_kept_one(), cmap, True)
            with pytest.raises(RuntimeError, match="256"):
                U.panoptic_fuse_up(sc, 4, s_stuff, r5, lg, ci, *_kept_one(), cmap)
    inputs = _small(3, S=161, C=9)
    s_stuff, r5, lg, ci, cmap = _fuse_args(inputs)
    with pytest.raises(RuntimeError, match="channel split"):
        U.panoptic_fuse_up(torch.zeros((1, 161, 8, 12), device='cuda'), 4, s_stuff, r5, lg, ci, *_kept_one(), cmap)
    for ms in (33, 1):
        inputs = _small(3, ms=ms)
        s_stuff, r5, lg, ci, cmap = _fuse_args(inputs)
        with pytest.raises(RuntimeError, match="mask.size"):
            _removal(U, inputs)
        with pytest.raises(RuntimeError, match="mask size"):
            U.panoptic_fuse(cu(inputs[0]), s_stuff, r5, lg, ci, *_kept_one(), cmap, True)
        with pytest.raises(RuntimeError, match="mask size"):
            U.panoptic_fuse_up(torch.zeros((1, 19, 8, 12), device='cuda'), 4, s_stuff, r5, lg, ci, *_kept_one(), cmap)
    torch.cuda.synchronize()
