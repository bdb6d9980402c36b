"""Box head and mask head (upsnet/models/rcnn.py:34-146). with_norm='none' (every shipped config) or 'group_norm':
the mask head's four convolutions lose their bias and are followed by nn.GroupNorm(32, dim_hidden), fc6 by
View -> GroupNorm(32, dim_hidden) -> View, on the per-sample forms of csrc/group_norm.hip (a ROI's result does not
depend on how many ROIs share the launch).

MI355X notes: FPNRoIAlign delivers channels-last pooled features straight from the kernel. The box head
consumes them without a transpose by using fc6's weight re-laid-out once to the (ph, pw, c) flatten
order (same dot products, different summation order); the mask head's convolutions take channels-last.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..config.config import config
from . import hipconv
from ..operators.modules.fpn_roi_align import FPNRoIAlign
from ..operators.modules.view import View


class MaskBranch(nn.Module):

    def __init__(self, num_classes, dim_in=256, dim_hidden=256, with_norm='none'):
        super(MaskBranch, self).__init__()
        norm = hipconv.head_norm(with_norm)
        self.roi_pooling = FPNRoIAlign(config.network.mask_size // 2, config.network.mask_size // 2,
                                       [1.0 / 4, 1.0 / 8, 1.0 / 16, 1.0 / 32], channels_last=True)
        if norm is not None:
            block = lambda cin: nn.Sequential(nn.Conv2d(cin, dim_hidden, 3, 1, 1, bias=False), norm(dim_hidden), nn.ReLU(inplace=True))
        else:
            block = lambda cin: nn.Sequential(nn.Conv2d(cin, dim_hidden, 3, 1, 1), nn.ReLU(inplace=True))
        self.mask_conv1 = block(dim_in)
        self.mask_conv2 = block(dim_hidden)
        self.mask_conv3 = block(dim_hidden)
        self.mask_conv4 = block(dim_hidden)
        self.mask_deconv1 = nn.Sequential(nn.ConvTranspose2d(dim_hidden, dim_hidden, 2, 2, 0), nn.ReLU(inplace=True))
        self.mask_score = nn.Conv2d(dim_hidden, num_classes, 1)
        self.initialize()

    def initialize(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                nn.init.kaiming_normal_(m.weight.data, mode='fan_in')
                if m.bias is not None:
                    m.bias.data.zero_()

    def forward(self, feat, rois):
        x = self.roi_pooling(feat, rois)
        for blk in (self.mask_conv1, self.mask_conv2, self.mask_conv3, self.mask_conv4):
            # Winograd form pinned whatever the ROI count: it varies per image and per pass, and the logits of a ROI must not
            # depend on how many other ROIs share the launch (the fused pipeline's single pass == the reference's two passes,
            # bit for bit) -- every 2x2 output tile is computed independently of the others, in a fixed K order
            # (bf16 mode: bf16 activations between the layers of the head, as in the backbone)
            if len(blk) == 3:   # conv -> GroupNorm -> ReLU: the pinned convolution, then the one-workgroup-per-ROI norm with the ReLU
                x = hipconv.norm(blk[1], hipconv.conv(blk[0], x, relu=False, winograd='always'), relu=True)
                continue
            x = hipconv.conv(blk[0], x, relu=True, winograd='always', out_dtype=hipconv.act_dtype())
        return hipconv.conv(self.mask_score, hipconv.deconv2x2(self.mask_deconv1[0], x, relu=True), pin=True)


FC_RELU_EPILOGUE = os.environ.get('UPSNET_FC_RELU', '1') != '0'


def _linear_relu(x, w, b):
    """relu(x @ w.T + b) (rcnn.py:137-140). On the GPU the ReLU rides in the library GEMM's epilogue (hipBLASLt, beside the bias it already
    applies there) instead of a separate elementwise launch per layer -- plumbing: the FC GEMMs are library work."""
    if FC_RELU_EPILOGUE and x.is_cuda and b is not None and x.dtype == torch.float32 and not torch.is_grad_enabled():
        return torch._addmm_activation(b, x, w.t(), use_gelu=False)
    return F.relu(F.linear(x, w, b), inplace=True)


class RCNN(nn.Module):

    def __init__(self, num_classes, num_reg_classes, pool_size=7, dim_in=256, dim_hidden=1024, with_fpn_pooling=True,
                 with_dpooling=False, with_adaptive_pooling=False, with_heavier_head=False, with_norm='none'):
        super(RCNN, self).__init__()
        assert with_fpn_pooling
        norm = hipconv.head_norm(with_norm)
        self.pool_size, self.dim_in = pool_size, dim_in
        self.roi_pooling = FPNRoIAlign(pool_size, pool_size, [1.0 / 4, 1.0 / 8, 1.0 / 16, 1.0 / 32], channels_last=True)
        if norm is not None:   # (the reference's indices: the norm is fc6.2)
            self.fc6 = nn.Sequential(nn.Linear((pool_size ** 2) * dim_in, dim_hidden), View(-1, dim_hidden, 1, 1), norm(dim_hidden),
                                     View(-1, dim_hidden), nn.ReLU(inplace=True))
        else:
            self.fc6 = nn.Sequential(nn.Linear((pool_size ** 2) * dim_in, dim_hidden), nn.ReLU(inplace=True))
        self.fc7 = nn.Sequential(nn.Linear(dim_hidden, dim_hidden), nn.ReLU(inplace=True))
        self.cls_score = nn.Linear(dim_hidden, num_classes)
        self.bbox_pred = nn.Linear(dim_hidden, num_reg_classes * 4)
        self.initialize()

    def initialize(self):
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.kaiming_uniform_(m.weight.data, a=1)
                if m.bias is not None:
                    m.bias.data.fill_(0)
        nn.init.normal_(self.cls_score.weight.data, 0, 0.01)
        self.cls_score.bias.data.fill_(0)
        nn.init.normal_(self.bbox_pred.weight.data, 0, 0.001)
        self.bbox_pred.bias.data.fill_(0)

    def _fc6_weight_nhwc(self, dtype=torch.float32):
        w, p = self.fc6[0].weight, self.pool_size
        relayout = lambda: w.detach().view(-1, self.dim_in, p, p).permute(0, 2, 3, 1).reshape(w.shape[0], -1).to(dtype).contiguous()
        return ops.cached_pack(self, 'fc6_nhwc', (w,), relayout, dtype)

    def forward(self, feat, rois, num_rois_dev=None):
        pool_feat = self.roi_pooling(feat, rois, num_rois_dev)            # channels_last [N,C,7,7]
        flat = pool_feat.permute(0, 2, 3, 1).reshape(pool_feat.size(0), -1)  # a view: physical (ph,pw,c) order
        if len(self.fc6) == 5:
            # fc6 -> GroupNorm -> ReLU: the library GEMM with its bias and no ReLU epilogue, then the rows form (half a wave per ROI)
            fc6 = hipconv.norm(self.fc6[2], F.linear(flat, self._fc6_weight_nhwc(), self.fc6[0].bias), relu=True)
        elif hipconv.PRECISION == 'bf16' and flat.is_cuda:
            # BASELINE configs[2]: the one large GEMM of the box head (1000 x 12544 x 1024, 26 GFLOP: 190 us as an fp32 library
            # GEMM) with bf16 operands, fp32 accumulation; bias + ReLU in fp32
            fc6 = F.linear(flat.to(torch.bfloat16), self._fc6_weight_nhwc(torch.bfloat16)).float()
            fc6 = F.relu_(fc6.add_(self.fc6[0].bias))
        else:
            fc6 = _linear_relu(flat, self._fc6_weight_nhwc(), self.fc6[0].bias)
        fc7 = _linear_relu(fc6, self.fc7[0].weight, self.fc7[0].bias) if isinstance(self.fc7, nn.Sequential) and len(self.fc7) == 2 else self.fc7(fc6)
        return {'cls_score': self.cls_score(fc7), 'bbox_pred': self.bbox_pred(fc7), 'fc_feat': fc7}
