"""CPU: the launch key, the launch signature and the greedy cover of the size sweeps (tests/test_size_sweep_gpu.py,
tests/test_size_sweep_lowprec_gpu.py) on hand-made trace records and a toy key table -- no device needed."""
import os
import sys
from types import SimpleNamespace

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_size_sweep_gpu import _fmt_key, _key, _signature, greedy_cover  # noqa: E402


def _conv_rec(m, n=1, hw=(20, 24), in_dtype=torch.float32, out_dtype=torch.float32, residual=None, form='igemm', relu=True):
    x = torch.zeros(n, m.in_channels, hw[0], hw[1], dtype=in_dtype)
    out = torch.zeros(n, m.out_channels, hw[0], hw[1], dtype=out_dtype)
    return dict(kind='conv', module=m, x=x, out=out, relu=relu, residual=residual, residual_up=False, form=form)


def _block(cin, cm, stride=1, proj=False):
    return SimpleNamespace(conv1=nn.Conv2d(cin, cm, 1, stride=stride, bias=False), conv2=nn.Conv2d(cm, cm, 3, padding=1, bias=False),
                           conv3=nn.Conv2d(cm, 4 * cm, 1, bias=False),
                           downsample=nn.Sequential(nn.Conv2d(cin, 4 * cm, 1, stride=stride, bias=False), nn.Identity()) if proj else None)


def _block_rec(blk, hw=(40, 48)):
    c1 = blk.conv1
    x = torch.zeros(1, c1.in_channels, hw[0], hw[1], dtype=torch.bfloat16)
    out = torch.zeros(1, blk.conv3.out_channels, hw[0] // c1.stride[0], hw[1] // c1.stride[0], dtype=torch.bfloat16)
    return dict(kind='block', module=blk, x=x, out=out, form='bottleneck_bf16' if blk.downsample is None else 'bottleneck_proj_bf16')


def test_the_key_of_an_fp32_record_is_the_nine_fields_of_the_fp32_sweep():
    m = nn.Conv2d(64, 128, 3, padding=1)
    rec = _conv_rec(m, residual=torch.zeros(1, 128, 20, 24), form='winograd tm32')
    assert _key(rec) == ('conv', 64, 128, (3, 3), (1, 1), True, True, False, 'winograd tm32')
    assert _signature(rec) == _key(rec) + ((1, 1), (1, 1), 1, ((1, 64, 20, 24),))
    dcn = dict(kind='dcn', module=m, xs=[torch.zeros(1, 64, 8, 8), torch.zeros(1, 64, 4, 4)], offsets=[None, None],
               outs=[torch.zeros(1, 128, 8, 8), torch.zeros(1, 128, 4, 4)], relu=True, form='dcn_fused multi')
    assert _key(dcn) == ('dcn', 64, 128, (3, 3), (1, 1), True, False, False, 'dcn_fused multi')
    assert _signature(dcn)[-1] == ((1, 64, 8, 8), (1, 64, 4, 4))
    # bf16x3: fp32 in, fp32 out -- the form string alone tells it from the fp32 launch
    assert _key(_conv_rec(m, form='bf16x3 conv_bf16<1,1,1>'))[:8] == _key(_conv_rec(m))[:8] and len(_key(_conv_rec(m, form='bf16x3 conv_bf16<1,1,1>'))) == 9


def test_dtypes_tell_launches_of_one_module_and_form_apart():
    m = nn.Conv2d(256, 256, 3, padding=1)
    form = 'bf16 conv3x3_wreg<8,2>'
    recs = {'f32->f32': _conv_rec(m, form=form),
            'f32->bf16': _conv_rec(m, out_dtype=torch.bfloat16, form=form),
            'bf16->f32': _conv_rec(m, in_dtype=torch.bfloat16, form=form),
            'bf16->bf16': _conv_rec(m, in_dtype=torch.bfloat16, out_dtype=torch.bfloat16, form=form),
            'bf16+bf16->bf16': _conv_rec(m, in_dtype=torch.bfloat16, out_dtype=torch.bfloat16, form=form,
                                         residual=torch.zeros(1, 256, 20, 24, dtype=torch.bfloat16)),
            'bf16+f32->bf16': _conv_rec(m, in_dtype=torch.bfloat16, out_dtype=torch.bfloat16, form=form, residual=torch.zeros(1, 256, 20, 24))}
    keys = {name: _key(rec) for name, rec in recs.items()}
    assert len(set(keys.values())) == len(keys), keys
    assert len(keys['f32->f32']) == 9 and all(k[:9] == keys['f32->f32'][:9] for n, k in keys.items() if '+' not in n)
    assert keys['bf16->f32'][9] == ('dtypes', ('bf16',), None, ('f32',)) and keys['bf16->bf16'][9] == ('dtypes', ('bf16',), None, ('bf16',))
    sigs = {name: _signature(rec) for name, rec in recs.items()}
    assert len(set(sigs.values())) == len(sigs)
    # the same launch on another map: same key, another signature; on the same map: the same signature
    other = _conv_rec(m, hw=(21, 24), in_dtype=torch.bfloat16, out_dtype=torch.bfloat16, form=form)
    assert _key(other) == keys['bf16->bf16'] and _signature(other) != sigs['bf16->bf16']
    assert _signature(_conv_rec(m, in_dtype=torch.bfloat16, out_dtype=torch.bfloat16, form=form)) == sigs['bf16->bf16']
    assert 'bf16 -> f32' in _fmt_key(keys['bf16->f32']) and '(+ f32)' in _fmt_key(keys['bf16+f32->bf16']) and '->' in _fmt_key(keys['f32->f32'])
    assert _fmt_key(keys['f32->f32']).endswith('[%s]' % form)
    deconv = dict(kind='deconv', module=nn.ConvTranspose2d(256, 256, 2, stride=2), x=torch.zeros(3, 256, 14, 14, dtype=torch.bfloat16),
                  out=torch.zeros(3, 256, 28, 28), relu=True, form='deconv2x2 bf16')
    assert _key(deconv)[9] == ('dtypes', ('bf16',), None, ('f32',)) and _signature(deconv)[-1] == ((3, 256, 14, 14),)


def test_a_one_launch_bottleneck_has_a_key_and_a_signature():
    ident, proj, proj2, wide = _block(256, 64), _block(64, 64, proj=True), _block(256, 128, stride=2, proj=True), _block(512, 128)
    keys = [_key(_block_rec(b)) for b in (ident, proj, proj2, wide)]
    assert len(set(keys)) == 4, keys
    k = keys[2]
    assert k[:9] == ('block', 256, 512, (3, 3), (2, 2), True, True, False, 'bottleneck_proj_bf16')
    assert k[9] == ('block', 128, (1, 1), (1, 1), (1, 1), True) and k[10] == ('dtypes', ('bf16',), None, ('bf16',))
    assert keys[0][9][-1] is False and keys[0][8] == 'bottleneck_bf16'
    assert _key(_block_rec(_block(256, 64))) == keys[0]      # another block of the same geometry: the same key
    assert _signature(_block_rec(ident)) == keys[0] + (((1, 256, 40, 48),),)
    assert _signature(_block_rec(ident, hw=(40, 56))) != _signature(_block_rec(ident))
    assert _fmt_key(k).startswith('block 256->512 k(3, 3) s(2, 2) relu + residual [bottleneck_proj_bf16]')
    # never mistaken for the separate launches of its layers
    assert _key(_conv_rec(ident.conv1, in_dtype=torch.bfloat16, out_dtype=torch.bfloat16, form='bf16 conv1x1_wreg<4,1>')) not in keys


def test_greedy_cover_with_forced_sizes_on_a_toy_key_table():
    table = {(800, 1344): {'a', 'b', 'c'}, (800, 800): {'a'}, (1344, 512): {'a', 'b'}, (608, 1344): {'c', 'd'}, (1344, 800): {'d'},
             (512, 1344): {'a', 'b', 'c'}}
    cover = greedy_cover(table)
    # most uncovered keys first, ties to the smallest size; then whatever brings the rest
    assert cover == [(512, 1344), (608, 1344)]
    assert set().union(*(table[s] for s in cover)) == set().union(*table.values())
    forced = [(1344, 512), (608, 1344), (800, 800)]
    cover = greedy_cover(table, forced)
    assert cover == [(512, 1344), (608, 1344), (1344, 512), (800, 800)]      # forced sizes follow, in their order, none twice
    assert greedy_cover({(1, 1): {'x'}, (2, 2): {'x'}}, [(2, 2)]) == [(1, 1), (2, 2)]
    assert greedy_cover({(1, 1): {'x', 'y'}, (2, 2): {'y', 'z'}, (3, 3): {'z'}}) == [(1, 1), (2, 2)]
    assert greedy_cover(table) == greedy_cover(dict(reversed(list(table.items()))))      # a function of the table, not of its order


def test_form_families_and_which_forms_count_as_reduced_precision():
    from test_size_sweep_lowprec_gpu import _family, _reduced
    assert _family('bf16 conv3x3_wreg<8,2>') == 'bf16 conv3x3_wreg' and _family('winograd splitk4') == 'winograd splitk'
    assert _family('winograd tm32 + tail tn32') == 'winograd tm + tail tn' and _family('winograd36 multi') == 'winograd36 multi'
    assert _reduced('bf16 conv_bf16<1,1,1>', 'bf16') and _reduced('dcn_fused multi bf16', 'bf16') and _reduced('bottleneck_proj_bf16', 'bf16')
    assert _reduced('bf16x3 conv_bf16<1,1,1>', 'bf16x3') and not _reduced('bf16x3 conv_bf16<1,1,1>', 'bf16')
    assert not _reduced('winograd36', 'bf16') and not _reduced('conv1x1 ksw 16x64', 'bf16x3')
