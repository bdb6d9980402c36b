"""Host-side regression table of the dense-convolution routing in upsnet_amd.models.hipconv: which launcher every layer of the two
presets takes on every map it can meet, with which arguments, under every flag, precision and knob.

The recorder replaces the `ops` convolution launchers and weight packers that hipconv calls with stubs that return meta tensors of the
right shape and log their own name, their scalar arguments and the shape / dtype of every tensor argument (bound to the real wrapper's
signature, so positional and keyword spellings log alike). It fixes the CU count at 256, lets meta tensors pass the `is_cuda` gate and
drives only hipconv.conv / conv_multi / conv_multi_cat with hipconv.TRACE on. No GPU, no library.

tests/golden/conv_routes.json.gz is the output of `python tests/conv_route_cases.py <path>` and tests/test_conv_routes_cpu.py compares the
working tree against it, case by case.
"""
import gzip
import inspect
import itertools
import json
import os
import sys

import torch
import torch.nn as nn

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_routes.json.gz')
F32, BF16 = torch.float32, torch.bfloat16
_DT = {F32: 'f32', BF16: 'bf16'}


class _OnDevice(torch.Tensor):
    """A meta tensor that answers is_cuda like a device tensor (views and casts of it stay of this class)."""
    is_cuda = True

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        with torch._C.DisableTorchFunctionSubclass():
            r = func(*args, **(kwargs or {}))
        return r.as_subclass(cls) if type(r) is torch.Tensor else r


def fmap(n, c, h, w, dtype=F32):
    return torch.empty(n, c, h, w, device='meta', dtype=dtype).as_subclass(_OnDevice)


# ----------------------------------------------------------------------------- layers: the conv geometries of CITYSCAPES_R50 / COCO_R101_DCN
def _layer(cin, cout, k, stride=1, pad=None, bias=True, dilation=1):
    return nn.Conv2d(cin, cout, k, stride=stride, padding=(k // 2 * dilation if pad is None else pad), dilation=dilation, bias=bias, device='meta')


IMAGE_SIZES = ((1024, 2048), (800, 1344), (256, 512))
ROI_MAPS = tuple((n, s, s) for s in (14, 28) for n in (1, 64, 83, 100, 143, 200))


def level(size, stride):
    return (1, -(-size[0] // stride), -(-size[1] // stride))


def _levels(strides):
    return tuple(level(size, st) for size in IMAGE_SIZES for st in strides)


ALL_LEVELS = _levels((4, 8, 16, 32, 64))

# name -> (module, maps (n, h, w) it is recorded on); the first `core` maps of each layer make the reduced set CORE
LAYERS = {}
CORE = []


def _add(name, module, maps, core=1):
    maps = tuple(dict.fromkeys(maps))
    LAYERS[name] = (module, maps)
    CORE.extend((name, mp) for mp in maps[:core])


for _stage, (_cin, _mid, _st) in enumerate(((64, 64, 4), (256, 128, 8), (512, 256, 16), (1024, 512, 32)), 2):
    _down = 1 if _stage == 2 else 2
    _in, _out = _levels((_st // _down, _st)), _levels((_st, 2 * _st))
    _add('res%d first conv1' % _stage, _layer(_cin, _mid, 1, stride=_down, bias=False), _in)
    _add('res%d proj' % _stage, _layer(_cin, 4 * _mid, 1, stride=_down, bias=False), _in)
    _add('res%d conv1' % _stage, _layer(4 * _mid, _mid, 1, bias=False), _out)
    _add('res%d conv2' % _stage, _layer(_mid, _mid, 3, bias=False), _out)
    _add('res%d conv3' % _stage, _layer(_mid, 4 * _mid, 1, bias=False), _out)
    if _stage > 2:
        _add('res%d offset' % _stage, _layer(_mid, 18, 3), _out)
        _add('fpn p%d lateral' % _stage, _layer(4 * _mid, 256, 1), _out)
    else:
        _add('fpn p2 lateral', _layer(256, 256, 1), _out)
_add('3x3 256 (fpn output, rpn, mask head)', _layer(256, 256, 3), ROI_MAPS[3:4] + ALL_LEVELS[:4] + ALL_LEVELS + ROI_MAPS, core=5)
_add('3x3 256 stride 2', _layer(256, 256, 3, stride=2), _levels((16, 32)))
for _c in (3, 12, 15, 60):
    _add('rpn head %d' % _c, _layer(256, _c, 1), _levels((4, 16, 64)))
_add('fcn offset 256', _layer(256, 18, 3), _levels((4, 8, 16, 32)))
_add('fcn offset 128', _layer(128, 18, 3), _levels((4, 8, 16, 32)))
_add('mask score 9', _layer(256, 9, 1), ROI_MAPS[9:] + ROI_MAPS)
_add('mask score 81', _layer(256, 81, 1), ROI_MAPS[9:] + ROI_MAPS)
_add('fcn score 19', _layer(512, 19, 1), _levels((4,)))
_add('fcn score 133', _layer(512, 133, 1), _levels((4,)))
UNSUPPORTED = {'dilated 3x3': _layer(256, 256, 3, dilation=2), 'cin 48': _layer(48, 64, 3), 'grouped': nn.Conv2d(256, 256, 3, padding=1, groups=2, device='meta')}

PAIRS = [(name, mp) for name, (_, maps) in LAYERS.items() for mp in maps]

WINOGRAD = (True, False, 'always', 'f2x2')
PIN = (False, True)
RESIDUAL = ('none', 'same', 'up')
OUT_DTYPE = (None, BF16)
# (PRECISION, input dtype, residual dtype)
FP32 = ('fp32', F32, F32)
LOWPREC = (('bf16x3', F32, F32), ('bf16', F32, F32), ('bf16', BF16, BF16))
MIXED = (('bf16', BF16, F32), ('bf16', F32, BF16), ('fp32', BF16, BF16))   # (the FPN laterals read a bf16 map and add an fp32 one)
# every knob flipped alone (module attributes of hipconv -> the value that is not the default), and the two forms that need two: the
# balanced 1x1 launch takes only layers the small-tile kernel leaves alone, the two-launch tail split only ROI batches the F(4x4) form does
KNOBS = tuple(((k, v),) for k, v in (('WINO36_SPLITK', True), ('WINO36_PREFIX', True), ('BALANCE', True), ('WINO36', False), ('WINO36_ROI', False),
                                     ('WINO_TAIL_SPLIT', False), ('WINO_TAIL_FUSED', False), ('KSW', False), ('KSW3', False), ('SPLITK', False),
                                     ('CONV1X1', False), ('WINOGRAD', False))) + (
    (('BALANCE', True), ('KSW', False)), (('WINO36_ROI', False), ('WINO_TAIL_FUSED', False)))
MODEL_FLAGS = ((True, False, 'none', None), (True, False, 'same', BF16), ('always', False, 'none', BF16), (True, True, 'up', None))

MULTI_LAYERS = ('3x3 256 (fpn output, rpn, mask head)', 'fcn offset 256', 'fcn offset 128', 'rpn head 3', 'rpn head 60', 'fpn p2 lateral', '3x3 256 stride 2')
MAP_LISTS = tuple(tuple(level(size, st) for st in strides) for size in IMAGE_SIZES for strides in ((4, 8, 16, 32, 64), (4, 8, 16, 32))) + (
    tuple(level(IMAGE_SIZES[0], st) for st in (4, 8, 16, 32, 64, 128)),)
CAT_PAIRS = (('rpn head 3', 'rpn head 12'), ('rpn head 15', 'rpn head 60'), ('rpn head 3', 'fcn offset 256'))


def grid():
    """Every case as a tuple (entry point, knob or None, (PRECISION, input dtype, residual dtype), ...)."""
    cases = []
    for name, mp in PAIRS:      # every flag on every layer and map, fp32 arithmetic
        cases += [('conv', None, FP32, name, mp, w, p, r, None) for w, p, r in itertools.product(WINOGRAD, PIN, RESIDUAL)]
    for name, mp in CORE:       # the reduced set: every flag and out_dtype in every precision and dtype mix
        cases += [('conv', None, prec, name, mp, w, p, r, od) for prec in (FP32,) + LOWPREC
                  for w, p, r, od in itertools.product(WINOGRAD, PIN, RESIDUAL, OUT_DTYPE) if (prec, od) != (FP32, None)]
        cases += [('conv', None, prec, name, mp, w, p, r, od) for prec in MIXED
                  for w, p, r, od in itertools.product((True, 'always'), PIN, RESIDUAL[1:], OUT_DTYPE)]
    for name, mp in PAIRS:      # every layer and map: the low-precision modes and every knob, with the flags the model uses
        cases += [('conv', None, prec, name, mp, w, p, r, od) for prec in LOWPREC for w, p, r, od in MODEL_FLAGS[:3]]
        cases += [('conv', knob, FP32, name, mp, w, p, r, None) for knob in KNOBS for w, p, r, _ in (MODEL_FLAGS[::2] if mp[0] > 1 else MODEL_FLAGS[:1])]
    for name, mp in CORE:
        cases += [('conv', knob, FP32, name, mp, w, p, r, None) for knob in KNOBS for w, p, r, _ in MODEL_FLAGS[1:]]
    for name in MULTI_LAYERS:
        for maps in MAP_LISTS:
            cases += [('conv_multi', knob, prec, name, maps, relu) for knob, prec in [(None, FP32)] + [(None, p) for p in LOWPREC] +
                      [(k, FP32) for k in KNOBS] for relu in (False, True)]
    for names in CAT_PAIRS:
        for maps in MAP_LISTS:
            cases += [('conv_multi_cat', knob, prec, names, maps, flat) for knob, prec in [(None, FP32)] + [(None, p) for p in LOWPREC] +
                      [(k, FP32) for k in KNOBS] for flat in (False, True)]
    for name in UNSUPPORTED:    # layers hipconv.supported rejects: raise, or the library path when that is allowed
        cases += [('fallback', allow, FP32, name, (1, 64, 128), kind) for allow in (False, True) for kind in ('device', 'cpu')]
    return list(dict.fromkeys(cases))   # (the reduced set is part of the full one: a case both sweeps name is recorded once)


def case_id(case):
    return json.dumps(case, default=lambda v: _DT.get(v, str(v)))


# ----------------------------------------------------------------------------- the stubs
def _desc(v):
    with torch._C.DisableTorchFunctionSubclass():
        return _desc1(v)


def _desc1(v):
    if isinstance(v, torch.Tensor):
        if type(v) is torch.Tensor and '_pack_tag' in v.__dict__:
            return v._pack_tag
        return '%s%s' % (_DT.get(v.dtype, str(v.dtype)), list(v.shape))
    if isinstance(v, (list, tuple)):
        return [_desc1(t) for t in v]
    if isinstance(v, torch.dtype):
        return _DT.get(v, str(v))
    return v


def _packed(tag, weight):
    t = torch.empty(0, device='meta')
    t._pack_tag = '<%s %s>' % (tag, list(weight.shape))
    return t


def _round_up(v, q):
    return -(-v // q) * q


# what each packer returns around its packed tensor(s): ops.py
_PACKERS = {
    'pack_conv_weight': lambda w: (_packed('direct', w), _round_up(w.shape[0], 32)),
    'pack_conv1x1_weight': lambda w: _packed('c1x1', w),
    'pack_conv1x1_ksw_weight': lambda w: _packed('ksw', w),
    'pack_conv3x3_ksw_weight': lambda w: _packed('ksw3', w),
    'pack_winograd_weight': lambda w, tn32=False: ((_packed('wino tn32', w), _round_up(w.shape[0], 32)) if tn32 else
                                                   (_packed('wino', w), 32 if w.shape[0] <= 32 else _round_up(w.shape[0], 64))),
    'pack_winograd36_weight': lambda w: (_packed('wino36', w), _round_up(w.shape[0], 64)),
    'pack_conv_weight_bf16': lambda w, split=True: (_packed('bf16 hi', w), _packed('bf16 lo', w) if split else None, _round_up(w.shape[0], 128)),
}
# launcher -> (kernel size, stride, padding) where its arguments do not carry them (ops.conv2d_nhwc is conv2d_nhwc_multi of one map and
# stays itself)
_LAUNCHERS = {
    'conv2d_nhwc_splitk': None, 'conv2d_nhwc_multi': None, 'conv2d_nhwc_bf16_multi': None,
    'conv1x1_frag': (1, None, 0), 'conv1x1_ksw': (1, None, 0), 'conv3x3_ksw': (3, 1, 1),
    'conv2d_winograd_multi': (3, 1, 1), 'conv2d_winograd_splitk': (3, 1, 1), 'conv2d_winograd_tail': (3, 1, 1),
    'conv2d_winograd36_multi': (3, 1, 1), 'conv2d_winograd36_splitk': (3, 1, 1),
}


def _signature(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def _bind(sig, args, kwargs):
    """{parameter: value} of a call, defaults filled in, in the order of the signature."""
    g = {name: (args[i] if i < len(args) else kwargs.get(name, default)) for i, (name, default) in enumerate(sig)}
    assert len(args) <= len(sig) and all(k in g for k in kwargs) and all(v is not inspect.Parameter.empty for v in g.values()), (sig, kwargs)
    return g


class Recorder:
    """Context manager: hipconv on stubs; `run(case)` -> the record of one case."""

    def __init__(self):
        from upsnet_amd import ops
        from upsnet_amd.models import hipconv
        self.ops, self.hipconv, self.log, self.saved = ops, hipconv, [], []

    def _set(self, obj, name, value):
        self.saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def __enter__(self):
        ops = self.ops
        for name, make in _PACKERS.items():
            self._set(ops, name, self._packer(name, _signature(getattr(ops, name)), make))
        for name, geom in _LAUNCHERS.items():
            self._set(ops, name, self._launcher(name, _signature(getattr(ops, name)), geom))
        self._set(ops, 'cached_pack', self._cached_pack)
        self._set(ops, 'last_kernel_form', lambda: 'instance')
        self._set(self.hipconv, '_cus', lambda device: 256)
        return self

    def __exit__(self, *exc):
        for obj, name, value in reversed(self.saved):
            setattr(obj, name, value)
        self.saved = []

    def _cached_pack(self, owner, slot, tensors, build, *extra):
        key = (id(owner), slot) + extra     # (cached for the length of one case: a second fetch packs nothing)
        if key not in self.packs:
            self.log.append(['cached_pack', slot, len(tensors), _desc(extra)])
            self.packs[key] = build()
        return self.packs[key]

    def _packer(self, name, sig, make):
        def stub(*a, **kw):
            g = _bind(sig, a, kw)
            self.log.append([name, _desc(list(g.items()))])
            return make(*g.values())
        return stub

    def _launcher(self, name, sig, geom):
        def stub(*a, **kw):
            g = _bind(sig, a, kw)
            self.log.append([name, _desc(list(g.items()))])
            k, st, pd = geom or (g['ksize'], g['stride'], g['pad'])
            st = g['stride'] if st is None else st
            dtype = g.get('out_dtype', F32)

            def out(x):
                return fmap(x.shape[0], g['cout'], (x.shape[2] + 2 * pd - k) // st + 1, (x.shape[3] + 2 * pd - k) // st + 1, dtype)
            if 'xs' in g:
                return list(g['outs']) if g.get('outs') is not None else [out(x) for x in g['xs']]
            return g['out'] if g.get('out') is not None else out(g['x'])
        return stub

    def _knobs(self, knob, prec):
        hc = self.hipconv
        undo = [('PRECISION', hc.PRECISION), ('TRACE', hc.TRACE), ('ALLOW_LIBRARY', hc.ALLOW_LIBRARY)]
        hc.PRECISION, hc.TRACE = prec, []
        for name, value in knob or ():
            undo.append((name, getattr(hc, name)))
            setattr(hc, name, value)
        return undo

    def run(self, case):
        hc = self.hipconv
        kind, knob, (prec, xdt, rdt) = case[:3]
        undo = self._knobs(None if kind == 'fallback' else knob, prec)
        self.log, self.packs = log, _ = [], {}
        n_fallbacks = len(hc.FALLBACKS)
        try:
            if kind == 'conv':
                name, (n, h, w), wino, pin, res, od = case[3:]
                m = LAYERS[name][0]
                st, k, pd = m.stride[0], m.kernel_size[0], m.padding[0]
                ho, wo = (h + 2 * pd - k) // st + 1, (w + 2 * pd - k) // st + 1
                r = {'none': None, 'same': fmap(n, m.out_channels, ho, wo, rdt), 'up': fmap(n, m.out_channels, (ho + 1) // 2, (wo + 1) // 2, rdt)}[res]
                ys = [hc.conv(m, fmap(n, m.in_channels, h, w, xdt), relu=(res != 'up'), residual=r, residual_up=(res == 'up'), winograd=wino, pin=pin,
                              out_dtype=od)]
            elif kind == 'conv_multi':
                name, maps, relu = case[3:]
                m = LAYERS[name][0]
                ys = hc.conv_multi(m, [fmap(n, m.in_channels, h, w, xdt) for n, h, w in maps], relu=relu)
            elif kind == 'conv_multi_cat':
                names, maps, flat = case[3:]
                ms = [LAYERS[name][0] for name in names]
                ys = hc.conv_multi_cat(ms, [fmap(n, ms[0].in_channels, h, w, xdt) for n, h, w in maps], return_flat=flat)
                ys = [ys[0], ys[1], ys[2]] if flat else ys
            else:
                name, (n, h, w), where = case[3:]
                hc.ALLOW_LIBRARY = knob
                m = UNSUPPORTED[name]
                if where == 'cpu':
                    torch.manual_seed(0)
                    m = nn.Conv2d(m.in_channels, m.out_channels, m.kernel_size, padding=m.padding, dilation=m.dilation, groups=m.groups)
                    ys = [hc.conv(m, torch.zeros(n, m.in_channels, 4, 4), relu=True)]
                else:
                    ys = [hc.conv(m, fmap(n, m.in_channels, h, w), relu=True)]
            rec = {'log': log, 'out': _desc(ys), 'fallbacks': len(hc.FALLBACKS) - n_fallbacks,
                   'trace': _desc([[t['form'], t['module'] is not None, t['x'], t['out'], t['relu'], t['residual'], t['residual_up'], ' '.join(t)]
                                   for t in hc.TRACE])}
        except Exception as e:   # noqa: BLE001 -- the exception type is the record
            rec = {'raises': type(e).__name__, 'log': log, 'fallbacks': len(hc.FALLBACKS) - n_fallbacks}
        finally:
            del hc.FALLBACKS[n_fallbacks:]
            for name, value in reversed(undo):
                setattr(hc, name, value)
        return json.dumps(rec, sort_keys=True)


def record_all():
    """-> (cases, one JSON record string per case) on the hipconv that is importable now."""
    cases = grid()
    with Recorder() as rec:
        return cases, [rec.run(c) for c in cases]


def dump(path):
    """The fixture: the case ids, the distinct records and, per case, the index of its record."""
    cases, records = record_all()
    table = {r: i for i, r in enumerate(dict.fromkeys(records))}
    doc = {'cases': [case_id(c) for c in cases], 'records': [json.loads(r) for r in table], 'index': [table[r] for r in records]}
    with open(path, 'wb') as f, gzip.GzipFile(filename='', mode='wb', fileobj=f, mtime=0) as z:
        z.write(json.dumps(doc, sort_keys=True, separators=(',', ':')).encode())
    return doc


def forms_of(records):
    return sorted({t[0] for r in records for t in r.get('trace', ())})


def load(path=FIXTURE):
    with gzip.open(path, 'rb') as z:
        return json.loads(z.read().decode())


if __name__ == '__main__':
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1] == '--time':
        for _ in range(int(sys.argv[2])):
            t0 = time.perf_counter()
            n = len(record_all()[1])
            print('%d cases %.3f s' % (n, time.perf_counter() - t0))
    else:
        doc = dump(sys.argv[1])
        forms = forms_of(doc['records'])
        print('%d cases, %d distinct records, %d forms: %s' % (len(doc['cases']), len(doc['records']), len(forms), forms))
