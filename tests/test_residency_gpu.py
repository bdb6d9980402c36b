"""GPU: a residency cap (csrc/residency.h) changes how many workgroups share a CU and nothing else -- for every covered kernel the
outputs under each cap are bit-identical to the uncapped launch, on the smallest shapes that reach every path (ragged last tiles in
both directions, more than one workgroup, every epilogue), and the whole model computes the same label map and boxes with the
table on. The cap is shown to have reached the launch by the dynamic LDS the launcher asked for."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FRAG, PAIR, PAIR32, KSW, WINO_32X64, WINO_32X32, DCN = range(7)
MAX_CAP = 8


def _lib():
    from upsnet_amd._lib import lib
    return lib()


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _nhwc(*shape, seed, scale=1.0):
    return _rand(*shape, seed=seed, scale=scale).contiguous(memory_format=torch.channels_last)


def _sweep(kernel, run, own_caps):
    """run() -> list of output tensors. own_caps: workgroups per CU the kernel's own LDS admits (a cap below it must add LDS)."""
    lib = _lib()
    try:
        assert lib.upsnet_residency_tuning(-1, 0) == 0
        ref = [t.clone() for t in run()]
        torch.cuda.synchronize()
        plain = lib.upsnet_residency_last_dynamic_lds()
        for cap in range(1, MAX_CAP + 1):
            assert lib.upsnet_residency_tuning(kernel, cap) == 0
            outs = run()
            torch.cuda.synchronize()
            asked = lib.upsnet_residency_last_dynamic_lds()
            assert (asked > plain) if cap < own_caps else (asked == plain), (cap, asked, plain)
            assert len(outs) == len(ref)
            for i, (o, r) in enumerate(zip(outs, ref)):
                assert torch.equal(o, r), "cap %d changed output %d" % (cap, i)
        # a cap on ANOTHER kernel leaves this launch alone
        assert lib.upsnet_residency_tuning(kernel, 0) == 0 and lib.upsnet_residency_tuning((kernel + 1) % 7, 1) == 0
        run()
        assert lib.upsnet_residency_last_dynamic_lds() == plain
    finally:
        lib.upsnet_residency_tuning(-1, 0)


@pytest.mark.parametrize("bn,cout", [(0, 96), (128, 160)], ids=["bn64", "bn128"])
def test_conv1x1_frag(bn, cout):
    """10 x 12 = 120 pixels: 2 m-tiles, the last ragged; 2 n-tiles, the last ragged; plain, residual, upsampled residual, split-K and
    the transposed-convolution scatter."""
    from upsnet_amd import ops
    x = _nhwc(1, 64, 10, 12, seed=1)
    w, b = _rand(cout, 64, 1, 1, seed=2, scale=0.1), _rand(cout, seed=3)
    res, res_up = _nhwc(1, cout, 10, 12, seed=4), _nhwc(1, cout, 5, 6, seed=5)
    wd, bd = _rand(64, 32, 2, 2, seed=6, scale=0.1), _rand(32, seed=7)
    wp = ops.pack_conv1x1_weight(w)
    wpd, bd4 = ops.pack_deconv2x2_weight_frag(wd, bd)

    def run():
        return [ops.conv1x1_frag(x, wp, b, cout, relu=True),
                ops.conv1x1_frag(x, wp, b, cout, relu=True, residual=res),
                ops.conv1x1_frag(x, wp, None, cout, residual=res_up, residual_up=True),
                ops.conv1x1_frag(x, wp, b, cout, stride=2),
                ops.conv1x1_frag(x, wp, b, cout, residual=res, ksplit=2),
                ops.deconv2x2_frag(x, wpd, bd4, 32, relu=True)]
    try:
        _lib().upsnet_conv1x1_tuning(bn)
        _sweep(FRAG, run, own_caps=10)      # 16 KiB of LDS: registers (4 per CU), not LDS, bound the plain launch
    finally:
        _lib().upsnet_conv1x1_tuning(0)


@pytest.mark.parametrize("c0,c1,kernel,own", [(64, 256, PAIR, 3), (128, 512, PAIR, 2), (256, 1024, PAIR32, 2)], ids=["res2", "res3", "res4"])
def test_conv1x1_pair(c0, c1, kernel, own):
    """8 x 16 = 128 pixels: one block boundary of the 64-pixel forms, three of the 32-pixel form."""
    from upsnet_amd import ops
    x, res = _nhwc(1, c0, 8, 16, seed=11), _nhwc(1, c1, 8, 16, seed=12)
    w3, b3 = _rand(c1, c0, 1, 1, seed=13, scale=0.1), _rand(c1, seed=14)
    w1, b1 = _rand(c0, c1, 1, 1, seed=15, scale=0.05), _rand(c0, seed=16)
    w3p, w1p = ops.pack_conv1x1_weight(w3), ops.pack_conv1x1_weight(w1)
    _sweep(kernel, lambda: list(ops.conv1x1_pair(x, res, w3p, b3, c1, w1p, b1, c0)), own_caps=own)


@pytest.mark.parametrize("tile,split_n,own", [((16, 64), False, 9), ((32, 32), False, 8), ((32, 64), False, 4), ((64, 64), False, 4),
                                              ((16, 256), True, 9), ((32, 128), True, 8), ((32, 256), True, 4)],
                         ids=["16x64k", "32x32k", "32x64k", "64x64k", "16x256n", "32x128n", "32x256n"])
def test_conv1x1_ksw(tile, split_n, own):
    """9 x 11 = 99 pixels, 288 output channels: ragged last tiles in both directions for every tile form; with a residual."""
    from upsnet_amd import ops
    x, res = _nhwc(1, 48, 9, 11, seed=21), _nhwc(1, 288, 9, 11, seed=22)
    w, b = _rand(288, 48, 1, 1, seed=23, scale=0.1), _rand(288, seed=24)
    wp = ops.pack_conv1x1_ksw_weight(w)
    _sweep(KSW, lambda: [ops.conv1x1_ksw(x, wp, b, 288, tile, relu=True, residual=res, split_n=split_n),
                         ops.conv1x1_ksw(x, wp, None, 288, tile, stride=2, split_n=split_n)], own_caps=own)


@pytest.mark.parametrize("cout,kernel", [(96, WINO_32X64), (24, WINO_32X32)], ids=["32x64", "32x32"])
def test_conv_wino16(cout, kernel):
    """A 10 x 18 map, Cin 32: 45 2x2 tiles = 2 workgroups of 32, the last ragged; a ragged last channel tile; with a residual; and a
    two-map launch."""
    from upsnet_amd import ops
    x, x2 = _nhwc(1, 32, 10, 18, seed=31), _nhwc(1, 32, 5, 9, seed=32)
    res = _nhwc(1, cout, 10, 18, seed=33)
    w, b = _rand(cout, 32, 3, 3, seed=34, scale=0.1), _rand(cout, seed=35)
    wp, ldw = ops.pack_winograd_weight(w)

    def run():
        return (ops.conv2d_winograd_multi([x], wp, ldw, b, cout, relu=True, residuals=[res])
                + ops.conv2d_winograd_multi([x, x2], wp, ldw, b, cout)
                + [ops.conv2d_winograd_splitk(x, wp, ldw, b, cout, 2, relu=True)])
    _sweep(kernel, run, own_caps=2)


def test_dcn_fused():
    """The two-level multi-map launch on 9 x 11 and 5 x 6 maps with random offsets (samples inside, on and outside the border)."""
    from upsnet_amd import ops
    xs = [_nhwc(1, 64, 9, 11, seed=41), _nhwc(1, 64, 5, 6, seed=42)]
    offs = [_nhwc(1, 18, 9, 11, seed=43, scale=2.0), _nhwc(1, 18, 5, 6, seed=44, scale=2.0)]
    w, b = _rand(160, 64, 3, 3, seed=45, scale=0.05), _rand(160, seed=46)
    wpack = ops.pack_dcn_weight(w, kind='frag')
    assert wpack[0] == 'frag'
    _sweep(DCN, lambda: ops.deform_conv_fused(xs, offs, wpack, b, 64, 160, (3, 3), (1, 1), (1, 1), (1, 1), relu=True), own_caps=4)


def test_whole_model_with_the_table_on():
    """One 256 x 512 forward with every covered kernel capped (1, then 2 workgroups per CU): label map and boxes of the uncapped forward."""
    from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50
    update_config_dict(CITYSCAPES_R50)
    from upsnet_amd.synthetic import build_model, make_image
    lib = _lib()
    model = build_model()
    data = make_image(256, 512, seed=0, device='cuda')
    keys = ('panoptic_outputs', 'pred_boxes', 'cls_probs', 'cls_inds', 'fcn_outputs')
    was = model.use_graph
    try:
        model.use_graph = False      # eager launches read the table as it stands (the graph path sets it only around its capture)
        with torch.no_grad():
            assert lib.upsnet_residency_tuning(-1, 0) == 0
            ref = {k: v.clone() for k, v in model(data).items() if k in keys}
            assert ref['pred_boxes'].shape[0] >= 1
            for cap in (1, 2, -1):
                assert lib.upsnet_residency_tuning(-1, cap) == 0
                out = model(data)
                for k in keys:
                    assert torch.equal(out[k], ref[k]), (cap, k)
    finally:
        lib.upsnet_residency_tuning(-1, 0)
        model.use_graph = was
