"""CPU: the heads built with with_norm = 'group_norm' have the reference's state-dict layout (tests/golden/gn_state_dict.json, recorded
from the reference's own modules by tests/golden/make_golden_gn.py), load a checkpoint with those keys strictly, refuse what is not
built ('batch_norm', GroupNorm under a bf16 convolution mode) with a reason, and the GroupNorm entry points validate their arguments
on the host."""
import ctypes
import json
import os
import warnings

import pytest
import torch

from conftest import ROOT

with open(os.path.join(ROOT, "tests", "golden", "gn_state_dict.json")) as _f:
    GOLDEN = json.load(_f)


def _builders():
    """The constructor arguments of tests/golden/make_golden_gn.py."""
    from upsnet_amd.config.config import config
    from upsnet_amd.models.fcn import FCNHead
    from upsnet_amd.models.fpn import FPN
    from upsnet_amd.models.rcnn import RCNN, MaskBranch
    from upsnet_amd.models.rpn import RPN
    assert config.network.mask_size == 28
    return {
        'FPN': lambda wn: FPN(feature_dim=256, with_norm=wn),
        'RPN': lambda wn: RPN(num_anchors=3, input_dim=256, with_norm=wn),
        'RCNN': lambda wn: RCNN(9, 9, dim_in=256, with_norm=wn),
        'MaskBranch': lambda wn: MaskBranch(9, dim_in=256, with_norm=wn),
        'FCNHead': lambda wn: FCNHead(256, 19, num_layers=3, with_norm=wn, upsample_rate=4),
    }


@pytest.fixture
def cityscapes():
    from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50, config
    update_config_dict(CITYSCAPES_R50)
    saved = {k: config.network[k] for k in ('fpn_with_norm', 'rcnn_with_norm', 'fcn_with_norm')}
    yield config
    for k, v in saved.items():
        setattr(config.network, k, v)


@pytest.mark.parametrize("with_norm", ['none', 'group_norm'])
@pytest.mark.parametrize("name", ['FPN', 'RPN', 'RCNN', 'MaskBranch', 'FCNHead'])
def test_state_dict_keys_match_the_reference(cityscapes, name, with_norm):
    assert not cityscapes.network.fpn_with_gap
    m = _builders()[name](with_norm)
    got = sorted((k, list(v.shape)) for k, v in m.state_dict().items())
    want = [(k, list(s)) for k, s in GOLDEN[name][with_norm]]
    assert got == want


def _set_norms(config, value):
    for k in ('fpn_with_norm', 'rcnn_with_norm', 'fcn_with_norm'):
        setattr(config.network, k, value)


def test_checkpoint_with_group_norm_keys_loads_strictly(cityscapes):
    from upsnet_amd.models.resnet_upsnet import resnet_50_upsnet
    _set_norms(cityscapes, 'group_norm')
    with torch.device('cpu'):
        model = resnet_50_upsnet()
    keys = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    # the heads' keys under their attribute names, as a reference checkpoint holds them (RPN is built without with_norm there too)
    nl = cityscapes.network.fcn_num_layers
    assert nl == 2
    for prefix, name in (('fpn.', 'FPN'), ('rcnn.', 'RCNN'), ('mask_branch.', 'MaskBranch')):
        for k, s in GOLDEN[name]['group_norm']:
            assert keys.get(prefix + k) == tuple(s), prefix + k
    for k in ('fcn_head.fcn_subnet.conv.0.1.weight', 'fcn_head.fcn_subnet.conv.1.1.bias', 'rpn.conv_proposal.0.weight'):
        assert k in keys, k
    assert 'rpn.conv_proposal.1.weight' not in keys
    g = torch.Generator().manual_seed(3)
    sd = {k: (torch.randn(v.shape, generator=g).to(v.dtype) if v.dtype.is_floating_point else v.clone()) for k, v in model.state_dict().items()}
    with torch.device('cpu'):
        fresh = resnet_50_upsnet()
    # nn.Module's own strict load (the model's loader is the reference's tolerant one: it warns instead of raising) ...
    res = torch.nn.Module.load_state_dict(fresh, sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    # ... and the model's loader, which must have nothing to warn about
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        fresh.load_state_dict(sd, resume=True, strict=True)
    assert torch.equal(fresh.fpn.fpn_p4_1x1[1].weight, sd['fpn.fpn_p4_1x1.1.weight'])
    assert torch.equal(fresh.rcnn.fc6[2].bias, sd['rcnn.fc6.2.bias'])
    # a 'none' model does not take it
    _set_norms(cityscapes, 'none')
    with torch.device('cpu'):
        plain = resnet_50_upsnet()
    with pytest.raises(RuntimeError):
        torch.nn.Module.load_state_dict(plain, sd, strict=True)


@pytest.mark.parametrize("name", ['FPN', 'RPN', 'RCNN', 'MaskBranch', 'FCNHead'])
def test_batch_norm_heads_are_refused_with_a_reason(cityscapes, name):
    with pytest.raises(NotImplementedError, match="BatchNorm2d"):
        _builders()[name]('batch_norm')
    with pytest.raises(AssertionError):
        _builders()[name]('layer_norm')


@pytest.mark.parametrize("precision", ['bf16', 'bf16x3'])
def test_group_norm_with_a_bf16_conv_precision_is_refused(cityscapes, monkeypatch, precision):
    from upsnet_amd.models import hipconv
    from upsnet_amd.models.resnet_upsnet import resnet_50_upsnet
    _set_norms(cityscapes, 'group_norm')
    with torch.device('cpu'):
        model = resnet_50_upsnet()
    monkeypatch.setattr(hipconv, 'PRECISION', precision)
    with pytest.raises(NotImplementedError, match="group_norm"):
        model.prepare_inference()
    monkeypatch.setattr(hipconv, 'PRECISION', 'fp32')
    model.prepare_inference()
    _set_norms(cityscapes, 'none')
    with torch.device('cpu'):
        plain = resnet_50_upsnet()
    monkeypatch.setattr(hipconv, 'PRECISION', precision)
    plain.prepare_inference()


def test_cpu_tensors_take_the_modules_own_group_norm(cityscapes):
    """CPU execution (the host path of the oracle and of the calibration) is the module itself + the same epilogue in torch."""
    from upsnet_amd.models import hipconv
    gn = torch.nn.GroupNorm(32, 128)
    g = torch.Generator().manual_seed(0)
    x, r = torch.randn(2, 128, 4, 6, generator=g), torch.randn(2, 128, 2, 3, generator=g)
    want = torch.relu(gn(x) + torch.nn.functional.interpolate(r, scale_factor=2, mode='nearest'))
    assert torch.equal(hipconv.norm(gn, x, relu=True, residual=r, residual_up=True), want)
    assert not hipconv.FALLBACKS or all('GroupNorm' not in f[0] for f in hipconv.FALLBACKS)
    ys = hipconv.norm_multi(gn, [x, x[:, :, :2]], relu=False)
    assert torch.equal(ys[0], gn(x)) and torch.equal(ys[1], gn(x[:, :, :2]))


def test_host_side_validation_without_gpu():
    """A null pointer, C = 96 and a residual of the wrong shape: error code + message, nothing touches the device."""
    from upsnet_amd import _lib, group_norm
    lib = _lib.lib()
    one = ctypes.c_void_p(16)
    ptrs = (ctypes.c_void_p * 1)(16)
    n, h, w = (ctypes.c_int * 1)(2), (ctypes.c_int * 1)(8), (ctypes.c_int * 1)(12)
    ok_res = ((ctypes.c_int * 1)(4), (ctypes.c_int * 1)(6))
    assert lib.upsnet_group_norm_chunk_pixels() == group_norm.chunk_pixels() > 0
    P = group_norm.chunk_pixels()
    assert lib.upsnet_group_norm_workspace_bytes(1, n, h, w) == 2 * 1 * 32 * 16
    assert lib.upsnet_group_norm_workspace_bytes(1, (ctypes.c_int * 1)(3), (ctypes.c_int * 1)(1), (ctypes.c_int * 1)(2 * P + 1)) == 3 * 3 * 32 * 16
    assert lib.upsnet_group_norm_workspace_bytes(6, n, h, w) == 0

    def call(x=ptrs, out=ptrs, C=256, gamma=one, beta=one, res=None, rh=None, rw=None, up=0, ws=one, nseg=1):
        return lib.upsnet_group_norm_nhwc_f32(None, nseg, x, out, n, h, w, C, gamma, beta, 1e-5, 0, res, rh, rw, up, ws)

    assert call(x=None) != 0 and b"null pointer" in lib.upsnet_last_error()
    assert call(gamma=None) != 0 and b"null pointer" in lib.upsnet_last_error()
    assert call(x=(ctypes.c_void_p * 1)(None)) != 0 and b"null pointer" in lib.upsnet_last_error()
    assert call(ws=None) != 0 and b"workspace" in lib.upsnet_last_error()
    for bad_c in (96, 64, 1152, 0):
        assert call(C=bad_c) != 0 and b"C %% 128" .replace(b"%%", b"%") in lib.upsnet_last_error(), bad_c
    assert call(nseg=6) != 0 and b"maps per launch" in lib.upsnet_last_error()
    assert call(x=(ctypes.c_void_p * 1)(20)) != 0 and b"aligned" in lib.upsnet_last_error()
    # residuals: same size, or half size with residual_up; anything else is refused
    assert call(res=ptrs, rh=(ctypes.c_int * 1)(8), rw=(ctypes.c_int * 1)(11)) != 0 and b"residual is 8 x 11" in lib.upsnet_last_error()
    assert call(res=ptrs, rh=ok_res[0], rw=ok_res[1], up=0) != 0 and b"residual" in lib.upsnet_last_error()
    assert call(res=ptrs, rh=h, rw=w, up=1) != 0 and b"upsampled residual" in lib.upsnet_last_error()
    assert call(res=ptrs) != 0 and b"res_height" in lib.upsnet_last_error()
    # the small form
    small = lambda x=one, C=256, hh=14, ww=14: lib.upsnet_group_norm_small_nhwc_f32(None, x, one, 3, hh, ww, C, one, one, 1e-5, 1)
    assert small(x=None) != 0 and b"null pointer" in lib.upsnet_last_error()
    assert small(C=96) != 0 and b"not supported" in lib.upsnet_last_error()
    assert small(hh=1, ww=P + 1) != 0 and b"at most" in lib.upsnet_last_error()
    # the Python side: an unsupported width goes the way of an unsupported convolution
    assert group_norm.supported(128) and group_norm.supported(1024) and not group_norm.supported(96) and not group_norm.supported(2048)
    assert not group_norm.supported(256, groups=16)
    with pytest.raises(Exception):
        group_norm.group_norm(torch.zeros(1, 256, 2, 2), torch.ones(256), torch.zeros(256))
