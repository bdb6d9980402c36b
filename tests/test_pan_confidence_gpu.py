"""GPU: the panoptic confidence kernels against tests/pan_confidence_ref.py.

ops.panoptic_fuse_up_conf: the label maps bit-equal to ops.panoptic_fuse_up's (and the oracle's), the confidence byte q within
|q - 255 conf_ref64| <= 0.5 + 255 * 1e-4 at every pixel. The bound is derived, not tuned: the logits are bit-identical to the oracle's
fp32 planes, so what remains is the fp32 exp (the argument z - z_max is exact or one rounding; the hardware exp2 after the multiply by
log2 e is good to a few ulps of a term that is at most 1), a sum of at most 160 + 256 + 1 positive terms (relative error at most about
417 * 2^-24 = 2.5e-5) and one division; conf <= 1, so 1e-4 absolute covers it four times over, and 0.5 is the rounding to a byte.
ops.pan_segment_scores, ops.pan_score_filter and ops.restore_plane_u8 are integer work: bit for bit. Every case runs on poisoned,
guard-banded memory of pattern A and then B: equal bytes, no band touched."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ops as oops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memguard  # noqa: E402
import pan_confidence_ref as ref  # noqa: E402
import panoptic_cases as pc  # noqa: E402
from conftest import gen_panoptic_maps  # noqa: E402

pytestmark = pytest.mark.gpu

QTOL = 0.5 + 255 * ref.TOL

SPECS = {pc.case_id(s): s for s in pc.FUSE_CASES}
UP = [n for n, (fn, args) in SPECS.items() if fn(*args)[0][7] % 4 == 0 and fn(*args)[0][8] % 4 == 0]
TINY = ['up_tiny-%d-%d-%d' % t for t in pc.UP_TINY]
CONF_CASES = UP + TINY + ['conf_crowd']


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def U():
    from upsnet_amd import ops
    return ops


# inputs and references are computed once per case and shared (never written to)
@functools.lru_cache(maxsize=None)
def _case(name):
    """(score [1,S,Hs,Ws], (rois5, prob, logit, cls, S, C, H, W), reference dict)"""
    if name == 'conf_crowd':
        score, *rest = ref.conf_crowd()[0]
    elif name.startswith('up_tiny-'):
        score, *rest = pc.up_tiny(*[int(v) for v in name.split('-')[1:]])[0]
    else:
        fn, args = SPECS[name]
        _, *rest = fn(*args)[0]
        S, H, W = rest[4], rest[6], rest[7]
        score = np.random.default_rng(sum(map(ord, name))).normal(0, 3, size=(1, S, H // 4, W // 4)).astype(np.float32)
    rois5, prob, logit, cls, S, C, H, W = rest
    return score, tuple(rest), ref.head_confidence(score, rois5, prob, logit, cls, S, C)


def test_the_case_list_is_the_issue_s():
    assert len(UP) == 11 and 'crowd-dropped' in UP and 'crowd-middle' in UP and 'kept_256' in UP
    assert [_case(n)[0].shape[2:] for n in TINY] == [(1, 1), (2, 3), (3, 70)] and _case(TINY[1])[0].shape[1] == 160


def _run_conf(U, name, nhwc, pattern=None):
    """(pan, sem, conf) of ops.panoptic_fuse_up_conf as numpy, after checking pan / sem against ops.panoptic_fuse_up; with `pattern`
    every allocation of the package is poisoned and banded and the inputs sit inside bands of poison."""
    score, (rois5, prob, logit, cls, S, C, H, W), want = _case(name)
    own = (lambda t: memguard.banded_copy(t, pattern)) if pattern else (lambda t: t)
    with (memguard.poisoned(pattern) if pattern else memguard.poisoned('A', modules=())):
        keep, num, real = U.mask_removal(cu(rois5[:, 1:]), cu(prob), cu(logit), cu(cls), C - 1, (H, W))
        assert np.array_equal(keep.cpu().numpy()[:int(num.item())], want['keep_inds'])
        sc = cu(score)
        if nhwc:
            sc = sc.contiguous(memory_format=torch.channels_last)
        args = (own(sc), 4, S - (C - 1), own(cu(rois5)), own(cu(logit)), own(cu(cls)), keep, num, real, own(cu(oops.class_mapping(S, C))))
        pan0, sem0 = U.panoptic_fuse_up(*args)
        pan, sem, conf = U.panoptic_fuse_up_conf(*args)
        assert conf.dtype == torch.uint8 and tuple(conf.shape) == (1, H, W)
        assert torch.equal(pan, pan0) and torch.equal(sem, sem0)
        return pan.cpu().numpy()[0], sem.cpu().numpy()[0], conf.cpu().numpy()[0]


def _check_conf(name, pan, sem, q):
    want = _case(name)[2]
    assert np.array_equal(pan, want['panoptic']) and np.array_equal(sem, want['sem'])
    err = np.abs(q.astype(np.float64) - 255.0 * want['conf'])
    print("%s: max |q - 255 conf_ref64| = %.6f (bound %.4f); conf in [%.4f, %.4f]" % (name, err.max(), QTOL, want['conf'].min(), want['conf'].max()))
    assert err.max() <= QTOL, (name, err.max(), np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("nhwc", [True, False])
@pytest.mark.parametrize("name", CONF_CASES)
def test_fuse_up_conf(U, name, nhwc):
    _check_conf(name, *_run_conf(U, name, nhwc))


@pytest.mark.parametrize("name", CONF_CASES)
def test_fuse_up_conf_on_poisoned_memory(U, name):
    for nhwc in (True, False):
        a = _run_conf(U, name, nhwc, 'A')
        b = _run_conf(U, name, nhwc, 'B')
        for x, y in zip(a, b):
            assert np.array_equal(x, y), "%s differs between the poison patterns" % name
        _check_conf(name, *a)


def test_fuse_up_conf_refuses_before_launching(U):
    score, (rois5, prob, logit, cls, S, C, H, W), _ = _case('kept_256')
    keep, num, real = U.mask_removal(cu(rois5[:, 1:]), cu(prob), cu(logit), cu(cls), C - 1, (H, W))
    cmap = cu(oops.class_mapping(S, C))
    with pytest.raises(RuntimeError, match="at most 256"):
        U.panoptic_fuse_up_conf(cu(score), 4, S - (C - 1), cu(np.concatenate([rois5, rois5[:1]])), cu(np.concatenate([logit, logit[:1]])),
                                cu(np.concatenate([cls, cls[:1]])), keep, num, real, cmap)
    with pytest.raises(RuntimeError, match="panoptic_fuse_up_conf"):
        U.panoptic_fuse_up_conf(cu(score), 2, S - (C - 1), cu(rois5), cu(logit), cu(cls), keep, num, real, cmap)


# ---------------------------------------------------------------------------------------------------- segment scores, filter, restore
SIZES = [(1, 1), (3, 5), (37, 53), (64, 2048), (128, 256)]


@functools.lru_cache(maxsize=None)
def _map(kind, H, W):
    """(pan_2ch uint8 [H,W,3], conf uint8 [H,W]): a gen_panoptic_maps scene through the oracle's get_unified_pan_result, cut to size;
    'noise': every pixel its own random key (the LDS tables overflow); 'full': the scene with a plane of all 255."""
    rng = np.random.default_rng(1000 * H + W)
    if kind == 'noise':
        pan = np.zeros((H, W, 3), np.uint8)
        pan[..., 0] = rng.integers(0, 256, (H, W))
        pan[..., 1] = rng.integers(0, 256, (H, W))
    else:
        seg, p, cls = gen_panoptic_maps(rng, max(H, 64), max(W, 96), 12)
        pan = np.ascontiguousarray(oops.get_unified_pan_result(seg, p, cls, 19, 9, 300)[:H, :W])
    conf = np.full((H, W), 255, np.uint8) if kind == 'full' else rng.integers(0, 256, (H, W)).astype(np.uint8)
    return pan, conf


MAPS = [('scene', H, W) for H, W in SIZES] + [('noise', 128, 256), ('noise', 37, 53), ('full', 128, 256)]
MAP_IDS = ['%s-%dx%d' % m for m in MAPS]


@functools.lru_cache(maxsize=None)
def _map_ref(kind, H, W):
    pan, conf = _map(kind, H, W)
    return ref.score_table(pan, conf), {T: ref.score_filter(pan, conf, T) for T in (0.0, 0.5, 1.0)}


def _run_scores(U, kind, H, W, pattern):
    """(table rows uint32 [n,3], {T: filtered map}, in-place filtered map at 0.5) with every buffer from poisoned, banded memory"""
    from upsnet_amd._lib import lib
    pan, conf = _map(kind, H, W)
    with memguard.poisoned(pattern, modules=()) as g:
        ws = g.empty((int(lib().upsnet_pan_segment_scores_workspace_bytes()),), dtype=torch.uint8, device='cuda')
        table = g.empty((int(lib().upsnet_pan_segment_scores_table_ints()),), dtype=torch.int32, device='cuda')
        src, c = memguard.banded_copy(cu(pan), pattern), memguard.banded_copy(cu(conf), pattern)
        got = U.pan_segment_scores(src, c, workspace=ws, table=table)
        assert got is table
        words = table.cpu().numpy().view(np.uint32)
        n = int(words[0])
        assert not words[1:4].any()
        rows = words[4:4 + 3 * n].reshape(n, 3).copy()
        outs = {}
        for T in (0.0, 0.5, 1.0):
            out = g.empty((H, W, 3), dtype=torch.uint8, device='cuda')
            assert U.pan_score_filter(src, table, T, out=out) is out
            outs[T] = out.cpu().numpy()
        assert np.array_equal(src.cpu().numpy(), pan) and np.array_equal(c.cpu().numpy(), conf)      # the inputs are not written
        assert U.pan_score_filter(src, table, 0.5, out=src) is src
        inplace = src.cpu().numpy()
    return rows, outs, inplace


@pytest.mark.parametrize("kind,H,W", MAPS, ids=MAP_IDS)
def test_segment_scores_and_filter_bit_for_bit_under_both_poisons(U, kind, H, W):
    want_rows, want_maps = _map_ref(kind, H, W)
    a = _run_scores(U, kind, H, W, 'A')
    b = _run_scores(U, kind, H, W, 'B')
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and all(np.array_equal(a[1][T], b[1][T]) for T in a[1])
    rows, outs, inplace = a
    assert rows.shape == want_rows.shape and np.array_equal(rows, want_rows)
    for T, m in outs.items():
        assert np.array_equal(m, want_maps[T]), (kind, H, W, T, int((m != want_maps[T]).sum()))
    assert np.array_equal(inplace, want_maps[0.5])
    assert np.array_equal(outs[0.0], _map(kind, H, W)[0])
    if kind == 'full':      # a plane of all 255: every score is 1, nothing goes even at T = 1
        assert np.array_equal(outs[1.0], _map(kind, H, W)[0]) and (rows[:, 2] == 255 * rows[:, 1]).all()
    if kind == 'noise' and H * W > 20000:
        assert len(rows) > 16000      # far more keys than a workgroup's LDS table holds


def test_scores_and_filter_defaults_allocate(U):
    pan, conf = _map('scene', 37, 53)
    table = U.pan_segment_scores(cu(pan), cu(conf))
    out = U.pan_score_filter(cu(pan), table, 0.5)
    assert np.array_equal(out.cpu().numpy(), _map_ref('scene', 37, 53)[1][0.5])
    with pytest.raises(ValueError):
        U.pan_score_filter(cu(pan), table, 1.5)
    with pytest.raises(ValueError):
        U.pan_segment_scores(cu(pan), cu(conf[:, :5].copy()))


@pytest.mark.parametrize("H,W,H0,W0", [(37, 53, 75, 107), (128, 256, 64, 100), (1, 1, 3, 5), (40, 96, 40, 96)])
def test_restore_plane_u8_is_indexing_with_the_tables(U, H, W, H0, W0):
    rng = np.random.default_rng(H0 * 1000 + W0)
    plane = rng.integers(0, 256, (H, W)).astype(np.uint8)
    ys, xs = np.sort(rng.integers(0, H, H0)).astype(np.int32), np.sort(rng.integers(0, W, W0)).astype(np.int32)
    want = plane[ys][:, xs]
    res = []
    for pattern in 'AB':
        with memguard.poisoned(pattern, modules=()) as g:
            out = g.empty((H0, W0), dtype=torch.uint8, device='cuda')
            src = memguard.banded_copy(cu(plane), pattern)
            assert U.restore_plane_u8(src, memguard.banded_copy(cu(ys), pattern), memguard.banded_copy(cu(xs), pattern), out=out) is out
            res.append(out.cpu().numpy())
    assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], want)
    assert np.array_equal(U.restore_plane_u8(cu(plane)[None], ys, xs).cpu().numpy(), want)
    wide = cu(np.concatenate([plane, plane], 1))
    assert np.array_equal(U.restore_plane_u8(wide[:, :W], ys, xs).cpu().numpy(), want)      # strided rows
