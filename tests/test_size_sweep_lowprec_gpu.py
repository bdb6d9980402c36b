"""GPU: every convolution launch of the bf16 and bf16x3 modes in float64 over the image sizes an evaluation set yields.

tests/test_size_sweep_gpu.py walks the size population in the fp32 mode. The two reduced-precision modes route the same way, and their
routing depends on the size even more: hipconv._use_bf16 decides per launch (a workgroup count) whether a layer runs on a bf16 kernel or on
an fp32 one, so which layers get rounded to bf16 at all moves with the image size; hipconv.use_block fuses a bottleneck into one launch only
on maps of at least 128 tiles; a layer fed bf16 activations or pinned (`always`) goes to a bf16 kernel however small its map is and meets
every edge-tile remainder of the population; and the kernel instance the library picks (conv3x3_wreg<8,2> / <2,1>, conv1x1_wreg<4,...>,
conv_bf16<...>: ops.last_kernel_form(), part of the form string) depends on the shape as well. tests/test_layerwise_gpu.py replays the bf16
mode at 256x512 / 1024x2048 (UPSNet-50) and 800x1333 (UPSNet-101-DCN) and the bf16x3 mode at 1024x2048 (UPSNet-50) only.

Same two passes as the fp32 sweep, per (preset, precision), on the sweep object of tests/test_size_sweep_gpu.py (its population, forced sizes,
greedy cover, key and signature -- here the key also carries the dtypes of a launch, and a one-launch bottleneck has a key):
  pass one   one traced eager forward per size; no fallback, no 'library' form, output at the padded size. Printed, not asserted: keys per
             form family, the layers whose precision changes over the population, the keys the sizes of the existing reduced-precision
             layerwise tests do not reach (asserted non-empty for bf16 on COCO).
  pass two   at every size of a cover of the keys, every launch in float64 from its recorded inputs; keys replayed == keys seen.
             bf16:   _replay_bf16 / _judge of tests/test_layerwise_gpu.py, unchanged: float64 on the bf16-rounded operands, bounds 'f32', 'b16',
                     'dcn16', 'chain' as stated there.
             bf16x3: _replay and the strict |err| <= 1e-4 + 1e-4 |ref| on the UNROUNDED operands, exactly as the fp32 sweep.
  the rest   bf16 only: the COCO sizes outside the cover (edge tiles), landscape and portrait apart.
End to end on UPSNet-101-DCN at the most extreme portrait size, per mode: check_taps stage-wise bit-identical, HIP-graph replay == eager,
and the (printed) agreement with the fp32 run of the same image.
"""
import os
import re
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import size_population as sp  # noqa: E402
from test_layerwise_gpu import _judge, _replay_bf16  # noqa: E402
from test_size_sweep_gpu import (WEIGHT_SEED, _OLD_SIZES_BY_PRECISION, _Sweep, _fmt_key, _forced, _key, _old_keys_of_both_presets, _population,  # noqa: E402
                                 _replay_sizes, _signature)

pytestmark = pytest.mark.gpu

PRECISIONS = ['bf16', 'bf16x3']
PRESETS = ['COCO_R101_DCN', 'CITYSCAPES_R50']


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """The four model objects (two presets x two precisions) and their workspaces live for this module only; whatever a test did, the
    session goes on in fp32 on the default preset."""
    from upsnet_amd.models import hipconv
    yield
    for key in [k for k in _Sweep._cache if k[1] != 'fp32']:
        del _Sweep._cache[key]
    torch.cuda.empty_cache()
    assert hipconv.PRECISION == 'fp32', hipconv.PRECISION


def _family(form):
    """Form string without what moves inside a family: template arguments, tile and split factors."""
    return re.sub(r'\b(splitk|tm|tn)\d+', r'\1', re.sub(r'<[^>]*>', '', form)).strip()


def _reduced(form, precision):
    """Did the launch run on a kernel of the reduced-precision mode (as opposed to an fp32 kernel)?"""
    return form.startswith(precision + ' ') or (precision == 'bf16' and form.endswith('bf16')) or form.startswith('bottleneck_')


def _describe(rec):
    xs = rec['xs'] if 'xs' in rec else [rec['x']]
    return '%s in %s' % (_fmt_key(_key(rec)), ', '.join(str(tuple(x.shape)) for x in xs))


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_pass_one_no_launch_leaves_the_hand_written_path_at_any_size(precision, preset):
    """One traced eager forward per size of the population in the mode (weight seed 235, image seed = index): no hipconv.FALLBACKS entry, no
    'library' form, output at the padded size (asserted by the sweep object). Prints the number of keys per form family, the layers that
    run on an fp32 kernel at some sizes and on a kernel of the mode at others, and the keys that none of the sizes of the reduced-precision
    tests of tests/test_layerwise_gpu.py reaches -- bf16 on COCO: there must be such keys, or this sweep adds nothing."""
    sweep = _Sweep.get(preset, precision)
    sweep.pass_one()
    sizes = sorted(sweep.keys_by_size)
    assert len(sizes) == len(_population(preset)) and (preset != 'COCO_R101_DCN' or len(sizes) >= 40)
    universe = set().union(*sweep.keys_by_size.values())
    everywhere = set.intersection(*sweep.keys_by_size.values())
    assert all('library' not in k[8] for k in universe)
    old = _old_keys_of_both_presets(precision)
    new = sorted(universe - old, key=_fmt_key)
    old_sizes = ', '.join('%s %s' % (p, ' '.join('%dx%d' % s for s in v)) for p, v in sorted(_OLD_SIZES_BY_PRECISION[precision].items()) if v)
    print("%s %s: %d sizes (%d portrait), %d keys seen, %d of them at every size, %d not at the sizes the %s layerwise tests run (%s)" %
          (preset, precision, len(sizes), sum(sp.is_portrait(s) for s in sizes), len(universe), len(everywhere), len(new), precision, old_sizes))
    families = {}
    for k in universe:
        families[_family(k[8])] = families.get(_family(k[8]), 0) + 1
    print("  keys per form family: %s" % ', '.join('%s %d' % kv for kv in sorted(families.items())))
    for k in sorted(universe - everywhere, key=_fmt_key):
        at = [s for s in sizes if k in sweep.keys_by_size[s]]
        print("  %-110s at %2d sizes%s" % (_fmt_key(k), len(at), '' if len(at) > 4 else ': ' + ', '.join('%dx%d' % s for s in at)))
    for k in new:
        at = [s for s in sizes if k in sweep.keys_by_size[s]]
        print("  new: %-105s at %2d sizes" % (_fmt_key(k), len(at)))
    # layers whose precision changes over the population
    by_layer = {}
    for s in sizes:
        for name, kind, form in sweep.forms_by_size[s]:
            by_layer.setdefault((name, kind), {}).setdefault(_reduced(form, precision), []).append((s, form))
    flips = sorted((nk, v) for nk, v in by_layer.items() if len(v) == 2)
    print("  %d layers run on an fp32 kernel at some sizes and on a %s kernel at others" % (len(flips), precision))
    for (name, kind), v in flips:
        at = {r: sorted(set(s for s, _ in v[r])) for r in (True, False)}
        few = at[True] if len(at[True]) <= len(at[False]) else at[False]
        print("    %-44s %-5s %s at %2d sizes: [%s]; %s at %2d: [%s]%s" %
              (name, kind, precision, len(at[True]), ', '.join(sorted(set(_family(f) for _, f in v[True]))), 'fp32', len(at[False]),
               ', '.join(sorted(set(_family(f) for _, f in v[False]))),
               '' if len(few) > 4 else ' (the fewer: %s)' % ', '.join('%dx%d' % s for s in few)))
    blocks = sorted((name, len(set(s for s, _ in v.get(True, [])))) for (name, kind), v in by_layer.items() if kind == 'block')
    partly = [(n, c) for n, c in blocks if c < len(sizes)]
    print("  %d bottlenecks run as one launch at some size, %d of them not at every size%s" %
          (len(blocks), len(partly), ''.join('\n    %-44s one launch at %2d of %d sizes' % (n, c, len(sizes)) for n, c in partly)))
    if preset == 'COCO_R101_DCN' and precision == 'bf16':
        assert new, "every bf16 key of the COCO population is reached at the sizes the layerwise tests already run"


def _replay_sizes_bf16(sweep, sizes):
    """_replay_sizes of the fp32 sweep for the bf16 mode: float64 replay of every launch at each padded size of `sizes` with _replay_bf16 (on the
    bf16-rounded operands) and its per-launch bound class, judged by _judge -- both of tests/test_layerwise_gpu.py, as its bf16 tests use them.
    A launch is skipped only if its signature was replayed at an EARLIER size. -> (table rows, violations, keys replayed)."""
    replayed_keys, bad, rows = set(), [], []
    sweep.configure()
    try:
        for padded in sizes:
            t0 = time.time()
            resized, seed = sweep.resized[padded]
            trace, _ = sweep.trace(resized[0], resized[1], seed=seed)
            assert set(_key(rec) for rec in trace) == sweep.keys_by_size[padded], padded      # the dispatch is a function of the shape
            n, worst_by, max_abs, here = 0, {}, 0.0, set()
            with torch.no_grad():
                for rec in trace:
                    sig = _signature(rec)
                    if sig in sweep.done:
                        continue
                    here.add(sig)
                    for ref, got, bound, extra in _replay_bf16(rec):
                        assert ref.shape == got.shape, (_describe(rec), ref.shape, got.shape)
                        worst, why = _judge(ref, got, bound, extra)
                        worst_by[bound] = max(worst_by.get(bound, 0.0), worst)
                        if ref.numel():
                            max_abs = max(max_abs, float((got.double() - ref).abs().max()))
                        if why is not None:
                            bad.append(('%dx%d' % padded, _describe(rec), why))
                        del ref
                    n += 1
                    replayed_keys.add(_key(rec))
            sweep.done |= here
            torch.cuda.synchronize()
            rows.append((padded, resized, len(trace), n, len(sweep.keys_by_size[padded]), worst_by, max_abs, time.time() - t0))
            del trace
    finally:
        sweep.restore()
    return rows, bad, replayed_keys


_CLASSES = ('f32', 'b16', 'dcn16', 'chain')


def _print_rows_bf16(rows):
    print("  padded size (image)        launches replayed  keys  worst err / bound: %s  max_abs    seconds" % '  '.join('%-5s' % c for c in _CLASSES))
    for padded, resized, total, n, nk, worst_by, max_abs, secs in rows:
        print("  %-10s (%-9s)  %4d  %4d      %4d                     %s  %.3g  %.2f" %
              ('%dx%d' % padded, '%dx%d' % resized, total, n, nk, '  '.join('%.3f' % worst_by[c] if c in worst_by else '  -  ' for c in _CLASSES),
               max_abs, secs))


def _print_rows_strict(rows):
    print("  padded size (image)        launches replayed  keys  worst err / bound  max_abs    forms")
    for padded, resized, total, n, nk, worst, max_abs, forms in rows:
        print("  %-10s (%-9s)  %4d  %4d      %4d  %.3f              %.3g  %s" %
              ('%dx%d' % padded, '%dx%d' % resized, total, n, nk, worst, max_abs, forms))


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_pass_two_every_launch_vs_fp64_at_a_covering_set_of_sizes(precision, preset):
    """Float64 replay of every launch of the mode at a set of sizes that covers every key of pass one (+ the forced sizes of the fp32 sweep);
    the set of keys replayed == the set of keys seen. bf16: against float64 on the bf16-rounded operands, each launch within the bound of
    its class (_replay_bf16: 'f32', 'b16', 'dcn16', 'chain'). bf16x3: against float64 on the unrounded operands, strictly within
    |err| <= 1e-4 + 1e-4 |ref| -- the bar of the fp32 kernels."""
    sweep = _Sweep.get(preset, precision)
    cover = sweep.cover()
    seen = set().union(*sweep.keys_by_size.values())
    forced = _forced(preset, _population(preset))
    assert all(s in cover for s in forced)
    sweep.done = set()
    t0 = time.time()
    rows, bad, replayed_keys = (_replay_sizes_bf16 if precision == 'bf16' else _replay_sizes)(sweep, cover)
    print("%s %s: cover of %d sizes out of %d (%d forced), %d keys seen, %d replayed, %.1f s" %
          (preset, precision, len(cover), len(sweep.keys_by_size), len(forced), len(seen), len(replayed_keys), time.time() - t0))
    (_print_rows_bf16 if precision == 'bf16' else _print_rows_strict)(rows)
    assert not bad, bad
    assert replayed_keys == seen, (sorted(seen - replayed_keys), sorted(replayed_keys - seen))


@pytest.mark.parametrize("orientation", ['landscape', 'portrait'])
def test_every_bf16_launch_vs_fp64_at_the_rest_of_the_coco_population(orientation):
    """bf16 mode: the pinned layers and the layers fed bf16 activations run on bf16 kernels at every map size, so within one form they meet
    every edge-tile remainder of the population. The COCO sizes the cover left out are replayed too -- same rule, same bounds, same
    de-duplication (after the cover when both tests run) -- landscape (the square included) and portrait apart. Measured: 0.27-0.38 s per
    size against 0.79 s for the first (nothing de-duplicated) size of the cover, 7.1 / 7.6 s per test: every size is kept, none thinned."""
    sweep = _Sweep.get('COCO_R101_DCN', 'bf16')
    cover = sweep.cover()
    portrait = orientation == 'portrait'
    rest = [s for s in sorted(sweep.keys_by_size) if s not in cover and sp.is_portrait(s) == portrait]
    mine = [s for s in sorted(sweep.keys_by_size) if sp.is_portrait(s) == portrait]
    assert len(rest) + sum(1 for s in cover if sp.is_portrait(s) == portrait) == len(mine) >= 20
    t0 = time.time()
    rows, bad, _ = _replay_sizes_bf16(sweep, rest)
    worst = {c: max(r[5].get(c, 0.0) for r in rows) for c in _CLASSES}
    print("COCO_R101_DCN bf16: the %d %s sizes outside the cover (all of them), worst error / bound %s, max_abs %.3g, %.1f s" %
          (len(rest), orientation, ' '.join('%s %.3f' % (c, worst[c]) for c in _CLASSES), max(r[6] for r in rows), time.time() - t0))
    _print_rows_bf16(rows)
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------------------- end to end
def _portrait_case(precision):
    """(sweep, (resized h, w), (padded h, w), image seed): UPSNet-101-DCN in the mode at the most extreme portrait size of the cover."""
    sweep = _Sweep.get('COCO_R101_DCN', precision)
    cover = sweep.cover()
    padded = _forced('COCO_R101_DCN', _population('COCO_R101_DCN'))[0]
    assert padded in cover and sp.is_portrait(padded)
    resized, seed = sweep.resized[padded]
    return sweep, resized, padded, seed


def _model_of(sweep):
    from upsnet_amd.synthetic import build_model
    if sweep.model is None:
        sweep.model = build_model(seed=WEIGHT_SEED)
    return sweep.model


@pytest.mark.parametrize("precision", PRECISIONS)
def test_stagewise_parity_and_agreement_on_a_portrait_image(precision):
    """UPSNet-101-DCN in the mode on one portrait image (the most extreme portrait size of the cover): every custom-op stage recomputed by the
    oracle from its tapped inputs bit for bit (check_taps; label map == oracle), at least one detection, output at the padded size. Prints
    the agreement of the semantic arg-max and of the panoptic label map with the fp32 run of the same image; no floor is asserted on it --
    none has been measured at these sizes (a later floor = the value recorded in DESIGN.md 2.2 minus the 0.03 margin of tests/test_model_gpu.py)."""
    from oracle.forward import check_taps
    from upsnet_amd.models import hipconv
    from upsnet_amd.synthetic import make_image
    sweep, (h, w), padded, seed = _portrait_case(precision)
    sweep.configure()
    try:
        model = _model_of(sweep)
        data = make_image(h, w, seed=seed, device='cuda')
        assert hipconv.PRECISION == 'fp32', hipconv.PRECISION
        with torch.no_grad():
            ref = {k: v.clone() for k, v in model(data).items()}
            hipconv.PRECISION = precision
            try:
                model.taps = {}
                out = model(data)
                taps = model.taps
            finally:
                hipconv.PRECISION, model.taps = 'fp32', None
        res = check_taps(taps, enable_void=model.enable_void)
        counts = res.pop('counts')
        assert all(res.values()), (res, counts)
        assert counts['label_mismatch'] == 0 and counts['n_det'] >= 1, counts
        assert tuple(out['panoptic_outputs'].shape) == (1,) + padded and tuple(taps['sem'].shape[-2:]) == padded
        assert torch.equal(out['panoptic_outputs'], taps['panoptic'])
        sem = float((out['fcn_outputs'] == ref['fcn_outputs']).float().mean())
        pan = float((out['panoptic_outputs'] == ref['panoptic_outputs']).float().mean())
        print('COCO_R101_DCN %s vs fp32 at %dx%d (padded %dx%d): semantic arg-max agreement %.4f, panoptic label-map agreement %.4f, n_det %d / %d, '
              'n_inst %d / %d, %s' % (precision, h, w, padded[0], padded[1], sem, pan, out['cls_inds'].numel(), ref['cls_inds'].numel(),
                                      out['panoptic_cls_inds'].numel(), ref['panoptic_cls_inds'].numel(), counts))
    finally:
        sweep.restore()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_hip_graph_replay_equals_eager_on_a_portrait_image(precision):
    """UPSNet-101-DCN in the mode at the most extreme portrait size through the HIP-graph path (two images in flight, two graph instances):
    every output of every step == the eager forward of that image in the same mode, on the keys the fp32 sweep's graph test compares."""
    from upsnet_amd.models import hipconv
    from upsnet_amd.synthetic import make_image
    sweep, (h, w), padded, seed = _portrait_case(precision)
    sweep.configure()
    try:
        model = _model_of(sweep)
        imgs = [make_image(h, w, seed=seed + j, device='cuda') for j in range(3)]
        keys = ('panoptic_outputs', 'pred_boxes', 'cls_probs', 'cls_inds', 'mask_probs', 'panoptic_cls_inds', 'fcn_outputs')
        was_graph, was_slots = model.use_graph, model.graph_slots
        assert hipconv.PRECISION == 'fp32', hipconv.PRECISION
        hipconv.PRECISION = precision
        try:
            with torch.no_grad():
                model.use_graph = False
                model._graphs.clear()
                eager = []
                for im in imgs:
                    out = model(im)
                    eager.append({k: out[k].clone() for k in keys})
                assert tuple(eager[0]['panoptic_outputs'].shape) == (1,) + padded
                model.use_graph, model.graph_slots = True, 2
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
            torch.cuda.synchronize()
            model._graphs.clear()
            model.use_graph, model.graph_slots = was_graph, was_slots
            hipconv.PRECISION = 'fp32'
    finally:
        sweep.restore()
