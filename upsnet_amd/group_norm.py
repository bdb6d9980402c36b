"""GroupNorm(32, C) on the HIP kernels of csrc/group_norm.hip (tensor plumbing only: allocation, layout views, stream).

    y = relu?( (x - mean_g) * rstd_g * gamma_c + beta_c  [+ residual | + nearest x2 upsampled residual] )

Three forms (include/upsnet_hip.h): `group_norm` / `group_norm_multi` (stats launch + apply launch, up to 5 maps sharing gamma / beta),
`group_norm_small` (one launch, one workgroup per sample of <= chunk_pixels() pixels: ROI maps) and, through the same entry point,
the rows form for [n, C] inputs (the box head's fc6). Nothing falls back to PyTorch; non-CUDA inputs raise. gamma / beta are read in
place; nothing is cached.
"""
import torch

from ._lib import aligned, check, int_array, lib, ptr, ptr_array, require_cuda, stream

GROUPS = 32
MAX_MAPS = 5


def supported(channels, groups=GROUPS):
    """The kernels' channel rule: 32 groups, C % 128 == 0, C <= 1024 (128, 256 and 1024 are the head widths of the model)."""
    return groups == GROUPS and channels % 128 == 0 and 0 < channels <= 1024


def chunk_pixels():
    """Pixels per chunk of the stats launch = the largest sample of the small form."""
    return int(lib().upsnet_group_norm_chunk_pixels())


def _nhwc(x):
    """[N,C,H,W] fp32 whose memory is NHWC-dense (no copy if it already is)."""
    if x.dtype != torch.float32:
        x = x.float()
    if not x.permute(0, 2, 3, 1).is_contiguous():
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return aligned(x)


def _affine(gamma, beta, channels):
    if gamma is None or beta is None or gamma.numel() != channels or beta.numel() != channels:
        raise RuntimeError("group_norm: gamma and beta must be [C] tensors")
    for t in (gamma, beta):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("group_norm: gamma / beta must be contiguous fp32 (they are read in place)")
    return aligned(gamma.detach()), aligned(beta.detach())


def _out_like(x):
    n, c, h, w = x.shape
    return torch.empty((n, h, w, c), dtype=torch.float32, device=x.device).permute(0, 3, 1, 2)


def group_norm_multi(xs, gamma, beta, eps=1e-5, relu=False, residuals=None, residual_up=False, outs=None):
    """GroupNorm(32, C) (+ residual, ReLU) of up to 5 maps [N_i,C,H_i,W_i] sharing gamma / beta: ONE stats launch and ONE apply launch,
    bit-identical to one call per map. residuals: None or one entry per map (None entries allowed), [N,C,H,W] or, with residual_up,
    [N,C,H/2,W/2] added through a nearest x2 upsampling. Returns channels_last outputs."""
    xs = list(xs)
    if not 1 <= len(xs) <= MAX_MAPS:
        raise RuntimeError("group_norm_multi: 1..%d maps per launch" % MAX_MAPS)
    require_cuda(gamma, beta, *xs)
    xs = [_nhwc(x) for x in xs]
    C = xs[0].shape[1]
    if any(x.dim() != 4 or x.shape[1] != C for x in xs):
        raise RuntimeError("group_norm_multi: maps must be [N,C,H,W] with one C")
    gamma, beta = _affine(gamma, beta, C)
    res = [None] * len(xs) if residuals is None else [None if r is None else _nhwc(r) for r in residuals]
    if len(res) != len(xs):
        raise RuntimeError("group_norm_multi: one residual entry per map")
    for x, r in zip(xs, res):
        if r is not None:
            require_cuda(r)
            if r.shape[0] != x.shape[0] or r.shape[1] != C:
                raise RuntimeError("group_norm_multi: residual %s does not match the map %s" % (tuple(r.shape), tuple(x.shape)))
    if outs is None:
        outs = [_out_like(x) for x in xs]
    else:
        for x, o in zip(xs, outs):
            if tuple(o.shape) != tuple(x.shape) or o.dtype != torch.float32 or not o.permute(0, 2, 3, 1).is_contiguous():
                raise RuntimeError("group_norm_multi: outs must be channels_last fp32 of the maps' shapes")
    batch, height, width = (int_array([x.shape[i] for x in xs]) for i in (0, 2, 3))
    ws = torch.empty((max(int(lib().upsnet_group_norm_workspace_bytes(len(xs), batch, height, width)), 16),), dtype=torch.uint8,
                     device=xs[0].device)
    has_res = any(r is not None for r in res)
    check(lib().upsnet_group_norm_nhwc_f32(
        stream(), len(xs), ptr_array(xs), ptr_array(outs), batch, height, width, int(C), ptr(gamma), ptr(beta), float(eps), int(bool(relu)),
        ptr_array(res) if has_res else None,
        int_array([0 if r is None else r.shape[2] for r in res]) if has_res else None,
        int_array([0 if r is None else r.shape[3] for r in res]) if has_res else None,
        int(bool(residual_up)), ptr(ws)), "group_norm_nhwc_f32")
    return outs


def group_norm(x, gamma, beta, eps=1e-5, relu=False, residual=None, residual_up=False, out=None):
    """group_norm_multi of one map."""
    return group_norm_multi([x], gamma, beta, eps, relu=relu, residuals=None if residual is None else [residual], residual_up=residual_up,
                            outs=None if out is None else [out])[0]


def group_norm_small(x, gamma, beta, eps=1e-5, relu=False):
    """GroupNorm(32, C) (+ ReLU) of samples of at most chunk_pixels() pixels in one launch, one workgroup per sample, the same reduction
    order whatever the batch size: x [N,C,H,W] (ROI maps; channels_last result) or [N,C] rows (half a wave per row; [N,C] result)."""
    require_cuda(x, gamma, beta)
    if x.dim() == 2:
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        x = aligned(x)
        n, C = x.shape
        h = w = 1
        out = torch.empty((n, C), dtype=torch.float32, device=x.device)
    elif x.dim() == 4:
        x = _nhwc(x)
        n, C, h, w = x.shape
        out = _out_like(x)
    else:
        raise RuntimeError("group_norm_small: x must be [N,C,H,W] or [N,C]")
    gamma, beta = _affine(gamma, beta, C)
    check(lib().upsnet_group_norm_small_nhwc_f32(stream(), ptr(x), ptr(out), int(n), int(h), int(w), int(C), ptr(gamma), ptr(beta), float(eps),
                                                 int(bool(relu))), "group_norm_small_nhwc_f32")
    return out
