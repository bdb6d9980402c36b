"""GPU: every convolution launch in float64 over the image sizes an evaluation set yields.

Which kernel a convolution runs on is decided per launch by models/hipconv.py from the map shape and the CU count (F(4x4) / F(2x2) Winograd,
32- / 64-tile form, split-K factor, small-tile 1x1 / 3x3 kernels, lean or general GEMM kernel, ...), and every threshold there is a workgroup
count: the choice moves with the image size. tests/test_layerwise_gpu.py and tests/test_trunk_gpu.py hold it to float64 at four sizes, all
landscape. A COCO evaluation set (upsnet_amd/evaluate.py) is dozens of padded sizes, half of them portrait (tests/size_population.py).

Pass one (cheap): one eager forward per size of the population with hipconv.TRACE on; every record becomes a key
(kind, Cin, Cout, kernel, stride, relu, residual, residual_up, form) -- the form string carries tile form and split factor. No launch may leave the
hand-written path at any size. (The sweep object takes a convolution precision: tests/test_size_sweep_lowprec_gpu.py walks the same
population in the bf16 and bf16x3 modes, where a key also carries the dtypes of a launch and a one-launch bottleneck has a key of its own;
the key of an fp32 record is the nine fields above.)
Pass two: sizes are picked by greedy set cover until every key of pass one is covered (plus the three most extreme portrait sizes and the size
with the smallest stride-32 map), and at each of them every launch is replayed in float64 from its recorded inputs exactly as
tests/test_layerwise_gpu.py does (its _replay, its bound |err| <= 1e-4 + 1e-4 |ref|). A launch is skipped only if the same module geometry,
input shape, flags and form were replayed at an earlier size. The set of keys replayed must equal the set of keys seen.
End to end at sizes of the cover: oracle.forward.check_taps stage-wise (proposals, detection selection, mask removal, panoptic and semantic maps
bit-identical -- the first portrait images those stages see in a model), the trunk logits against float64 with the strict list of
tests/test_trunk_gpu.py, and HIP-graph replay == eager on a portrait image.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import size_population as sp  # noqa: E402
from test_layerwise_gpu import TOL, _describe, _replay  # noqa: E402

pytestmark = pytest.mark.gpu

WEIGHT_SEED = 235

# the sizes tests/test_layerwise_gpu.py and tests/test_trunk_gpu.py run each preset at (fp32 mode)
_OLD_SIZES = {'CITYSCAPES_R50': [(256, 512), (1024, 2048)], 'COCO_R101_DCN': [(200, 333), (800, 1333), (1024, 2048)]}
# ... and the sizes the reduced-precision tests of tests/test_layerwise_gpu.py replay each preset at
_OLD_SIZES_BY_PRECISION = {'fp32': _OLD_SIZES,
                           'bf16': {'CITYSCAPES_R50': [(256, 512), (1024, 2048)], 'COCO_R101_DCN': [(800, 1333)]},
                           'bf16x3': {'CITYSCAPES_R50': [(1024, 2048)], 'COCO_R101_DCN': []}}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """The two model objects (and the workspaces of ~60 image sizes) live for this module only."""
    yield
    _Sweep._cache.clear()
    torch.cuda.empty_cache()


def _population(preset):
    return sp.one_per_padded(sp.coco_padded_sizes()) if preset == 'COCO_R101_DCN' else sp.cityscapes_sizes()


def _forced(preset, sizes):
    """Members of the cover whatever the keys say: the three most extreme portrait sizes and the size with the smallest stride-32 map
    (COCO); the portrait frame (Cityscapes)."""
    padded = [p for _, p in sizes]
    portrait = sorted((p for p in padded if sp.is_portrait(p)), key=lambda p: (-p[0] / float(p[1]), p))
    if preset != 'COCO_R101_DCN':
        return portrait[:1]
    smallest = min(padded, key=lambda p: ((p[0] // 32) * (p[1] // 32), p))
    return portrait[:3] + [smallest]


_DTYPE_NAMES = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16', torch.float64: 'f64'}


def _dtypes(rec):
    """() for a launch that reads and writes fp32 only (every launch of the fp32 and bf16x3 modes); else (('dtypes', inputs, residual,
    outputs),): a bf16-in / fp32-out launch is another kernel instantiation than a bf16-in / bf16-out one."""
    name = lambda t: _DTYPE_NAMES.get(t.dtype, str(t.dtype))
    ins = tuple(name(x) for x in (rec['xs'] if 'xs' in rec else [rec['x']]))
    outs = tuple(name(y) for y in (rec['outs'] if 'outs' in rec else [rec['out']]))
    res = None if rec.get('residual') is None else name(rec['residual'])
    if all(d == 'f32' for d in ins + outs) and res in (None, 'f32'):
        return ()
    return (('dtypes', ins, res, outs),)


def _key(rec):
    """(kind, Cin, Cout, kernel, stride, relu, residual, residual_up, form) -- followed, for the launches the reduced-precision modes add, by
    what tells them apart: the geometry of a one-launch bottleneck (kind 'block': no single conv module) and the dtypes of a launch that
    does not read and write fp32 only. The key of an fp32 record is the nine fields alone."""
    m = rec['module']
    if rec['kind'] == 'block':     # relu(conv3(relu(conv2(relu(conv1(x))))) + shortcut(x)) as one launch: m is the bottleneck
        c1, c2, c3 = m.conv1, m.conv2, m.conv3
        return (('block', c1.in_channels, c3.out_channels, tuple(c2.kernel_size), tuple(c1.stride), True, True, False, rec['form']) +
                (('block', c1.out_channels, tuple(c1.kernel_size), tuple(c2.stride), tuple(c2.padding), m.downsample is not None),) + _dtypes(rec))
    return (rec['kind'], m.in_channels, m.out_channels, tuple(m.kernel_size), tuple(m.stride), bool(rec.get('relu', False)),
            rec.get('residual') is not None, bool(rec.get('residual_up', False)), rec['form']) + _dtypes(rec)


def _signature(rec):
    """What a launch is, apart from its values: module geometry, input shape(s) and dtypes, flags, form."""
    m = rec['module']
    xs = rec['xs'] if 'xs' in rec else [rec['x']]
    if rec['kind'] == 'block':     # (its key holds the geometry of conv1 / conv2 / the projection)
        return _key(rec) + (tuple(tuple(x.shape) for x in xs),)
    return _key(rec) + (tuple(m.padding), tuple(m.dilation), int(getattr(m, 'groups', 1)), tuple(tuple(x.shape) for x in xs))


def _fmt_key(k):
    dt = next((e for e in k[9:] if e[0] == 'dtypes'), None)
    return "%s %d->%d k%s s%s%s%s [%s]%s" % (k[0], k[1], k[2], k[3], k[4], ' relu' if k[5] else '',
                                             ' + up(residual)' if k[7] else (' + residual' if k[6] else ''), k[8],
                                             '' if dt is None else ' %s%s -> %s' % ('+'.join(dt[1]), '' if dt[2] is None else ' (+ %s)' % dt[2], '+'.join(dt[3])))


def greedy_cover(keys_by_size, forced=()):
    """Sizes (in the order picked) whose keys cover the union: the size with the most uncovered keys first, ties to the smallest size;
    then the forced sizes that the cover did not need."""
    universe = set().union(*keys_by_size.values())
    chosen, covered = [], set()
    while covered != universe:
        best = max(sorted(keys_by_size), key=lambda s: len(keys_by_size[s] - covered))
        assert keys_by_size[best] - covered
        chosen.append(best)
        covered |= keys_by_size[best]
    return chosen + [s for s in forced if s not in chosen]


class _Sweep(object):
    """One model object of a preset (seeded weights) in one convolution precision and what pass one saw on it. Built once per
    (preset, precision) and process."""
    _cache = {}

    def __init__(self, preset, precision='fp32'):
        self.preset, self.precision = preset, precision
        self.model, self.keys_by_size, self.old_keys, self.resized, self.done = None, None, None, {}, set()
        self.forms_by_size = {}      # padded size -> {(layer name, kind, form)}: which kernel each layer of the model ran on there

    @classmethod
    def get(cls, preset, precision='fp32'):
        if (preset, precision) not in cls._cache:
            cls._cache[(preset, precision)] = cls(preset, precision)
        return cls._cache[(preset, precision)]

    def configure(self):
        from upsnet_amd.config import config as cfgmod
        cfgmod.update_config_dict(getattr(cfgmod, self.preset))

    @staticmethod
    def restore():
        from upsnet_amd.config.config import update_config_dict, CITYSCAPES_R50
        update_config_dict(CITYSCAPES_R50)

    def trace(self, h, w, seed):
        """One eager forward of an h x w image in this sweep's precision with hipconv.TRACE on -> (records, output). Call between
        configure() and restore(). The session's precision (fp32) is put back whatever happens."""
        from upsnet_amd.models import hipconv
        from upsnet_amd.synthetic import build_model, make_image
        assert hipconv.PRECISION == 'fp32', hipconv.PRECISION      # nothing before this call leaked a reduced precision
        if self.model is None:
            self.model = build_model(seed=WEIGHT_SEED)
        data = make_image(h, w, seed=seed, device='cuda')
        hipconv.TRACE, n_fallbacks = [], len(hipconv.FALLBACKS)
        saved, hipconv.PRECISION, ran = hipconv.PRECISION, self.precision, None
        try:
            with torch.no_grad():
                out = self.model(data)
            torch.cuda.synchronize()
            trace, ran = hipconv.TRACE, hipconv.PRECISION
        finally:
            hipconv.TRACE, hipconv.PRECISION = None, saved
        assert ran == self.precision, (ran, self.precision)
        assert len(hipconv.FALLBACKS) == n_fallbacks, ((h, w), hipconv.FALLBACKS[n_fallbacks:])
        assert not any(rec['form'] == 'library' for rec in trace), (h, w)
        return trace, out

    def pass_one(self):
        if self.keys_by_size is not None:
            return
        self.configure()
        try:
            keys_by_size = {}
            for i, (resized, padded) in enumerate(_population(self.preset)):
                trace, out = self.trace(resized[0], resized[1], seed=i)
                assert trace and tuple(out['panoptic_outputs'].shape[1:]) == padded, (resized, padded, len(trace))
                keys_by_size[padded] = set(_key(rec) for rec in trace)
                self.resized[padded] = (resized, i)
                names = {id(m): n for n, m in self.model.named_modules()}
                self.forms_by_size[padded] = set((names.get(id(rec['module']), '?'), rec['kind'], rec['form']) for rec in trace)
                del trace, out
            old = set()
            for j, (h, w) in enumerate(_OLD_SIZES_BY_PRECISION[self.precision][self.preset]):
                trace, _ = self.trace(h, w, seed=100 + j)
                old |= set(_key(rec) for rec in trace)
                del trace
            self.keys_by_size, self.old_keys = keys_by_size, old
        finally:
            self.restore()

    def cover(self):
        self.pass_one()
        return greedy_cover(self.keys_by_size, _forced(self.preset, _population(self.preset)))


def _old_keys_of_both_presets(precision='fp32'):
    old = set()
    for preset in sorted(_OLD_SIZES):
        sweep = _Sweep.get(preset, precision)
        sweep.pass_one()
        old |= sweep.old_keys
    return old


@pytest.mark.parametrize("preset", ['COCO_R101_DCN', 'CITYSCAPES_R50'])
def test_pass_one_no_launch_leaves_the_hand_written_path_at_any_size(preset):
    """One traced eager forward per size of the population (weight seed 235, image seed = index): no hipconv.FALLBACKS entry, no 'library'
    form, output at the padded size. Prints how many keys each form family has and how the choice moves over the sizes."""
    sweep = _Sweep.get(preset)
    sweep.pass_one()
    sizes = sorted(sweep.keys_by_size)
    assert len(sizes) == len(_population(preset)) and (preset != 'COCO_R101_DCN' or len(sizes) >= 40)
    universe = set().union(*sweep.keys_by_size.values())
    everywhere = set.intersection(*sweep.keys_by_size.values())
    assert all('library' not in k[8] for k in universe)
    print("%s: %d sizes (%d portrait), %d keys seen, %d of them at every size, %d not at the sizes the layerwise tests run (%s)" %
          (preset, len(sizes), sum(sp.is_portrait(s) for s in sizes), len(universe), len(everywhere), len(universe - sweep.old_keys),
           ', '.join('%dx%d' % s for s in _OLD_SIZES[preset])))
    for k in sorted(universe - everywhere, key=_fmt_key):
        at = [s for s in sizes if k in sweep.keys_by_size[s]]
        print("  %-88s at %2d sizes%s" % (_fmt_key(k), len(at), '' if len(at) > 4 else ': ' + ', '.join('%dx%d' % s for s in at)))


def _replay_sizes(sweep, sizes):
    """Float64 replay of every launch at each padded size of `sizes`, in that order, as tests/test_layerwise_gpu.py does it: same recorded
    inputs, same recorded offsets, its _replay, its bound. A launch is skipped only if its signature was replayed at an EARLIER size
    (sweep.done; the signatures of a size join it after that size). -> (table rows, violations, keys replayed)."""
    replayed_keys, bad, rows = set(), [], []
    sweep.configure()
    try:
        for padded in sizes:
            resized, seed = sweep.resized[padded]
            trace, _ = sweep.trace(resized[0], resized[1], seed=seed)
            assert set(_key(rec) for rec in trace) == sweep.keys_by_size[padded], padded      # the dispatch is a function of the shape
            n, forms, worst_size, max_abs, here = 0, set(), 0.0, 0.0, set()
            with torch.no_grad():
                for rec in trace:
                    sig = _signature(rec)
                    if sig in sweep.done:
                        continue
                    here.add(sig)
                    refs, gots = _replay(rec)
                    for ref, got in zip(refs, gots):
                        assert ref.shape == got.shape, (_describe(rec), ref.shape, got.shape)
                        err = (got.double() - ref).abs()
                        worst = float((err / (TOL + TOL * ref.abs())).max()) if err.numel() else 0.0
                        worst_size = max(worst_size, worst)
                        max_abs = max(max_abs, float(err.max()) if err.numel() else 0.0)
                        if not worst <= 1.0:
                            bad.append(('%dx%d' % padded, _describe(rec), round(worst, 3), float(err.max()), float(ref.abs().max())))
                    n += 1
                    forms.add(rec['form'])
                    replayed_keys.add(_key(rec))
                    del refs, gots
            sweep.done |= here
            rows.append((padded, resized, len(trace), n, len(sweep.keys_by_size[padded]), worst_size, max_abs, sorted(forms)))
            del trace
    finally:
        sweep.restore()
    return rows, bad, replayed_keys


def _print_rows(rows):
    print("  padded size (image)        launches replayed  keys  worst err / bound  max_abs    forms")
    for padded, resized, total, n, nk, worst, max_abs, forms in rows:
        print("  %-10s (%-9s)  %4d  %4d      %4d  %.3f              %.3g  %s" %
              ('%dx%d' % padded, '%dx%d' % resized, total, n, nk, worst, max_abs, forms))


@pytest.mark.parametrize("preset", ['COCO_R101_DCN', 'CITYSCAPES_R50'])
def test_pass_two_every_launch_vs_fp64_at_a_covering_set_of_sizes(preset):
    """Float64 replay of every launch at a set of sizes that covers every key of pass one. The set of keys replayed == the set of keys seen
    (nothing is left out); every launch strictly within |err| <= 1e-4 + 1e-4 |ref| of its float64 value on the recorded inputs (deformable
    layers at their recorded offsets). COCO: the cover reaches keys that none of the sizes of the existing layerwise tests reaches."""
    sweep = _Sweep.get(preset)
    cover = sweep.cover()
    seen = set().union(*sweep.keys_by_size.values())
    forced = _forced(preset, _population(preset))
    assert all(s in cover for s in forced)
    sweep.done = set()
    rows, bad, replayed_keys = _replay_sizes(sweep, cover)
    old = _old_keys_of_both_presets()
    new = sorted(seen - old, key=_fmt_key)
    print("%s: cover of %d sizes out of %d (%d forced), %d keys seen, %d replayed, %d not reached by the sizes of the existing layerwise tests" %
          (preset, len(cover), len(sweep.keys_by_size), len(forced), len(seen), len(replayed_keys), len(new)))
    _print_rows(rows)
    for k in new:
        print("  new: %-88s first at %s" % (_fmt_key(k), '%dx%d' % next(s for s in cover if k in sweep.keys_by_size[s])))
    assert not bad, bad
    assert replayed_keys == seen, (sorted(seen - replayed_keys), sorted(replayed_keys - seen))
    if preset == 'COCO_R101_DCN':
        assert new, "every key of the COCO population is reached at the sizes the layerwise tests already run"


def test_every_launch_vs_fp64_at_the_rest_of_the_coco_population():
    """The cover holds every (layer, form) choice; it does not hold every tile remainder: within one form the stride-32 maps are 16..42 wide
    and high, and edge tiles are where a kernel goes wrong. A replay costs about a third of a second per size, so the sizes the cover left
    out are replayed too, same rule, same bound, same de-duplication (after the cover when both tests run)."""
    sweep = _Sweep.get('COCO_R101_DCN')
    cover = sweep.cover()
    rest = [s for s in sorted(sweep.keys_by_size) if s not in cover]
    assert len(rest) + len(cover) == len(sweep.keys_by_size) >= 40
    rows, bad, _ = _replay_sizes(sweep, rest)
    print("COCO_R101_DCN: the %d sizes outside the cover, worst error / bound %.3f, max_abs %.3g" %
          (len(rest), max(r[5] for r in rows), max(r[6] for r in rows)))
    _print_rows(rows)
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------------------- end to end
def _end_to_end_size(slot):
    """(preset, (resized h, w), (padded h, w), image seed) of one end-to-end case. The COCO cases are members of the cover: the most extreme
    portrait size, the smallest map, and the portrait size the greedy cover picked first (the one that brings the most keys; if it picked
    none beyond the forced ones, the second most extreme)."""
    if slot == 'cityscapes_portrait':
        return 'CITYSCAPES_R50', (2048, 1024), (2048, 1024), 2
    sweep = _Sweep.get('COCO_R101_DCN')
    cover = sweep.cover()
    forced = _forced('COCO_R101_DCN', _population('COCO_R101_DCN'))
    if slot == 'most_extreme_portrait':
        padded = forced[0]
    elif slot == 'smallest_map':
        padded = forced[3]
    else:
        assert slot == 'portrait_of_the_cover'
        padded = next((s for s in cover if sp.is_portrait(s) and s != forced[0]), forced[1])
    assert padded in cover
    resized, seed = sweep.resized[padded]
    return 'COCO_R101_DCN', resized, padded, seed


@pytest.mark.parametrize("slot", ['most_extreme_portrait', 'portrait_of_the_cover', 'smallest_map', 'cityscapes_portrait'])
def test_stagewise_parity_and_trunk_logits_at_sizes_of_the_cover(slot):
    """Every custom-op stage bit-identical to the oracle (check_taps: proposals, the two detection selections, mask removal, panoptic and
    semantic maps; label_mismatch == 0) with the output at the padded size, and the trunk logits within 1e-4 of the float64 execution with the
    strict list of tests/test_trunk_gpu.py -- on portrait images (H > W: the ROI ordering table cuts its image stripes along the height)
    and on the smallest map of the population."""
    from oracle.forward import check_taps
    from test_trunk_gpu import _STRICT_C1, _STRICT_C2, _run, _summary
    from upsnet_amd.config import config as cfgmod
    preset, (h, w), padded, seed = _end_to_end_size(slot)
    assert slot == 'smallest_map' or h > w
    sweep = _Sweep.get(preset)
    sweep.configure()
    try:
        from upsnet_amd.synthetic import build_model, make_image
        model = sweep.model if sweep.model is not None else build_model(seed=WEIGHT_SEED)
        data = make_image(h, w, seed=seed, device='cuda')
        model.taps = {}
        try:
            with torch.no_grad():
                out = model(data)
            taps = model.taps
        finally:
            model.taps = None
        res = check_taps(taps, enable_void=model.enable_void)
        counts = res.pop('counts')
        print('%s %dx%d (padded %dx%d): %s' % (preset, h, w, padded[0], padded[1], counts))
        assert all(res.values()), (res, counts)
        assert counts['label_mismatch'] == 0 and counts['n_det'] >= 1, counts
        assert tuple(out['panoptic_outputs'].shape) == (1,) + padded and tuple(taps['sem'].shape[-2:]) == padded
        assert torch.equal(out['panoptic_outputs'], taps['panoptic'])
        del taps, out
    finally:
        sweep.restore()
    rep = _run(getattr(cfgmod, preset), h, w, seed=seed, strict=_STRICT_C2 if preset == 'COCO_R101_DCN' else _STRICT_C1, report_only=['fcn_score'],
               weight_seed=WEIGHT_SEED)
    _summary(rep, '%s %dx%d' % (preset, h, w))


def test_hip_graph_replay_equals_eager_on_a_portrait_image():
    """UPSNet-101-DCN at the most extreme portrait size of the population through the HIP-graph path (two images in flight, two graph instances):
    every output of every step == the eager forward of that image, on the keys test_mixed_stream_at_real_sizes_graph_replay_equals_eager compares."""
    preset, (h, w), padded, seed = _end_to_end_size('most_extreme_portrait')
    sweep = _Sweep.get(preset)
    sweep.configure()
    try:
        from upsnet_amd.synthetic import build_model, make_image
        model = sweep.model if sweep.model is not None else build_model(seed=WEIGHT_SEED)
        imgs = [make_image(h, w, seed=seed + j, device='cuda') for j in range(3)]
        keys = ('panoptic_outputs', 'pred_boxes', 'cls_probs', 'cls_inds', 'mask_probs', 'panoptic_cls_inds', 'fcn_outputs')
        was_graph, was_slots = model.use_graph, model.graph_slots
        try:
            with torch.no_grad():
                model.use_graph = False
                eager = []
                for im in imgs:
                    out = model(im)
                    eager.append({k: out[k].clone() for k in keys})
                assert tuple(eager[0]['panoptic_outputs'].shape) == (1,) + padded
                model.use_graph, model.graph_slots = True, 2
                model._graphs.clear()
                for _ in range(3 * model.graph_slots):      # eager, eager, capture -- per instance
                    model(imgs[0])
                pending = []
                for step in range(9):
                    j = step % 3
                    pending.append((j, model.forward_async(imgs[j])))
                    if len(pending) >= 2:
                        jj, handle = pending.pop(0)
                        out = handle.result()
                        for k in keys:
                            assert torch.equal(out[k], eager[jj][k]), (step, jj, k)
                for jj, handle in pending:
                    out = handle.result()
                    for k in keys:
                        assert torch.equal(out[k], eager[jj][k]), (jj, k)
                graphs = sum(1 for slots in model._graphs.values() for ent in slots['slots'] if 'graph' in ent)
                assert graphs == model.graph_slots, graphs      # the portrait shape really ran as graph replays
        finally:
            model._graphs.clear()
            model.use_graph, model.graph_slots = was_graph, was_slots
    finally:
        sweep.restore()
