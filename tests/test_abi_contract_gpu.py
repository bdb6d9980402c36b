"""GPU: what the package's wrappers hand across the C ABI (tests/abiguard.py), on the test bodies of the poisoned-memory sweep.

a. Canonical sweep. Every case of tests/test_poisoned_memory_gpu.py (CASES) and of EXTRA_CASES below -- the wrappers that call the
   library but allocate nothing, which that table does not list -- runs its existing test body once under abiguard.guard(), on
   ordinary memory: the body's own reference comparison stays in force, no pointer argument may break a rule, and every entry point the
   case lists must have been called. Two more cases run an eager forward of each model preset, and one an eager forward at the
   smallest size of tests/size_population.py at which a pyramid level has an odd pixel count. The guard's alignment rule holds every
   pointer of these runs to 16 bytes, so they check every carve-out the package makes inside its own buffers.

b. Form sweep. For each wrapper (a module-level function whose body calls an upsnet_* symbol with a pointer parameter) the arguments
   of its first call in its case are captured (tensors cloned) and the call is replayed under the guard with ONE tensor argument at a
   time replaced by a variant of equal values:
     strided  a view that is contiguous in no memory format (the innermost dimension of the physical layout taken ::2 out of a buffer
              twice as long); tensors of at most one element have none;
     dtype    float32 -> float64, int32 -> int64, int64 -> int32, bool -> uint8; other dtypes have none;
     offset   the same sizes and strides one element into a buffer one element longer, so that the address is a multiple of the element
              size and not of 16; only a tensor without elements has none.
   Every argument is cloned afresh for each replay. A replay must end as
     same     the returned tensors (their defined region) and every tensor argument after the call (workspaces apart: scratch) are
              bitwise what the canonical replay gave, and no rule was broken, or
     refused  ValueError / TypeError / RuntimeError out of the wrapper before any entry point with a pointer parameter was called
              (a size query such as upsnet_*_workspace_bytes takes no pointer and launches nothing: many wrappers need its answer
              to judge the workspace they were given, so it does not count).
   An AbiViolation, a different result or an exception after a launch fails the test: the wrapper is to be fixed.
   The guard raises before the library is entered, so no variant reaches a kernel mistyped, dangling, mis-strided or off alignment
   (abiguard.UNALIGNED lists the few parameters whose kernels were read and found to access them at element width only: their offset
   variant does reach the kernel, and must come out `same`); variants never change a value.

c. A form that a wrapper's docstring promises must come out `same` (PROMISED). tools/abi_forms.py writes the outcome table of this
   sweep for two trees side by side (profiles/abi_forms.txt): no row may go from same to refused.
"""
import collections
import contextlib
import importlib
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abiguard  # noqa: E402
import memguard  # noqa: E402
import test_poisoned_memory_gpu as sweep  # noqa: E402
from test_poisoned_memory_gpu import CASES, Case, case_call  # noqa: E402

pytestmark = pytest.mark.gpu


def _c(id, module, test, entries, **kwargs):
    return Case(id, module, test, kwargs, tuple(entries))


# wrappers that call the library with pointers and allocate nothing (their callers hand them outputs and workspaces)
EXTRA_CASES = [
    _c('x_deform_col2im', 'test_backward_gpu', 'test_deform_col2im', ('ops.deform_col2im', 'ops.mod_deform_col2im'),
       C=4, H=15, W=15, pad=1, stride=2, dil=1, dg=1),
    _c('x_deform_col2im_coord', 'test_backward_gpu', 'test_deform_col2im_coord_bit_exact',
       ('ops.deform_col2im_coord', 'ops.mod_deform_col2im_coord'), C=4, H=15, W=15, pad=1, stride=2, dil=1, dg=1),
    _c('x_roi_align_backward', 'test_backward_gpu', 'test_roi_align_backward', ('ops.roi_align_backward',)),
    _c('x_nms_host_2', 'test_ops_gpu', 'test_gpu_nms_bitexact', ('ops.nms_host',), n=2, thresh=0.5),
    _c('x_boundary_pq_hand', 'test_boundary_pq_gpu', 'test_hand_case', ('ops.pq_boundary_accumulate',)),
    _c('x_boundary_map_17x33', 'test_boundary_pq_gpu', 'test_panoptic_boundary_bits', ('ops.pan_boundary_map',), H=17, W=33, d=2),
    _c('x_segment_scores_37x53', 'test_pan_confidence_gpu', 'test_segment_scores_and_filter_bit_for_bit_under_both_poisons',
       ('ops.pan_segment_scores', 'ops.pan_score_filter'), kind='noise', H=37, W=53),
    _c('x_restore_both_maps_37x53', 'test_abi_contract_gpu', 'test_restore_label_maps_takes_both_maps_and_device_tables',
       ('ops.restore_label_maps',)),
    _c('x_restore_plane_37x53', 'test_pan_confidence_gpu', 'test_restore_plane_u8_is_indexing_with_the_tables', ('ops.restore_plane_u8',),
       H=37, W=53, H0=75, W0=107),
    _c('x_vis_font', 'test_vis_gpu', 'test_odd_sizes_and_detection_counts_match_restatement', ('vis.font_table',), H=33, W=65, n=9),
    _c('x_track_step', 'test_pan_track_gpu', 'test_hand_cases_equal_the_restatement', ('ops._pan_track_step',), name='three_frames'),
    _c('x_stable_colours', 'test_pan_track_gpu', 'test_stable_colours_equal_the_host_statement', ('ops.pan_stable_colors',), H=37, W=53),
    _c('x_video_eval', 'test_video_pq_gpu', 'test_hand_cases_equal_the_restatement', ('ops.video_eval_frame', 'ops.video_eval_end'),
       name='short'),
    _c('x_mots_eval', 'test_mots_gpu', 'test_sequence_with_zero_scored_frames', ('ops.mots_eval_frame', 'ops.mots_eval_end')),
    _c('x_rle_transitions', 'test_mots_gpu', 'test_rle_transitions_equal_numpy', ('ops.pan_rle_transitions',), name='edge'),
    _c('x_proposal_recall', 'test_proposal_recall_gpu', 'test_poisoned_memory', ('ops.proposal_recall',)),
    _c('x_cs_expand_37x53', 'test_cityscapes_inst_format_gpu', 'test_poisoned_guard_banded_memory', ('cityscapes_inst_format._expand_into',),
       size=(37, 53), one_bit=True),
]

ALL_CASES = list(CASES) + EXTRA_CASES

# entry -> the case whose first call the form sweep captures, where the first case that lists the entry does not hand it every
# argument as a tensor (restore_pil_shrink calls restore_label_maps without a pano map and with numpy tables)
FORM_CASE = {'ops.restore_label_maps': 'x_restore_both_maps_37x53'}


def test_restore_label_maps_takes_both_maps_and_device_tables():
    """ops.restore_label_maps with a pano map and int32 DEVICE index tables, which no other test body hands it: out[y, x] = low byte of
    src[y_ofs[y], x_ofs[x]] (include/upsnet_hip.h) against plain indexing, and host tables give the same bytes. The body of the case
    that the form sweep replays for this wrapper (FORM_CASE)."""
    from upsnet_amd import ops
    g = torch.Generator().manual_seed(5)
    H, W, H0, W0 = 37, 53, 75, 107
    sseg = torch.randint(0, 300, (1, H, W), generator=g).cuda()          # (int64; values past 255: the low byte is kept)
    pano = torch.randint(0, 70000, (1, H, W), generator=g).cuda()
    ys = torch.randint(0, H, (H0,), generator=g, dtype=torch.int32)
    xs = torch.randint(0, W, (W0,), generator=g, dtype=torch.int32)
    want_s = (sseg[0].cpu()[ys.long()][:, xs.long()] & 255).to(torch.uint8)
    want_p = (pano[0].cpu()[ys.long()][:, xs.long()] & 255).to(torch.uint8)
    got_s, got_p = ops.restore_label_maps(sseg, pano, ys.cuda(), xs.cuda())
    assert got_s.dtype == torch.uint8 and torch.equal(got_s.cpu(), want_s) and torch.equal(got_p.cpu(), want_p)
    host_s, host_p = ops.restore_label_maps(sseg, pano, ys, xs)
    assert torch.equal(host_s.cpu(), want_s) and torch.equal(host_p.cpu(), want_p)

# functions that call the library with a pointer and are neither an entry of a case nor replayed by the form sweep, and why
EXCLUDED = {}

# the methods of stateful objects among the entries: what they hand to the library comes from the object's state (its workspace,
# its accumulators, the frame before), not from the arguments of one call, so a replay of captured arguments is not the call again.
# The canonical sweep runs them; the free functions they go through (ops.video_eval_frame, ops._pan_track_step, ...) are replayed.
FORM_EXCLUDED_REASON = "method of a stateful object: its pointers come from the object's state, not from the captured arguments"

# (entry point, argument, variant) -> the promise in the wrapper's docstring: must come out `same`
# ('rows' and 'host' are variants made for these promises alone: rows at a wider pitch with contiguous columns, a host tensor)
PROMISED = {
    ('ops.restore_label_maps', 'sseg', 'rows'): "rows may be strided, columns contiguous",
    ('ops.restore_label_maps', 'pano', 'rows'): "rows may be strided, columns contiguous",
    ('ops.restore_label_maps', 'y_ofs', 'host'): "y_ofs / x_ofs int32 index tables (host or device)",
    ('ops.restore_label_maps', 'x_ofs', 'host'): "y_ofs / x_ofs int32 index tables (host or device)",
    ('ops.restore_plane_u8', 'plane', 'rows'): "rows may be strided, columns contiguous",
    ('ops.restore_plane_u8', 'y_ofs', 'host'): "the same index tables (host or device)",
    ('ops.restore_plane_u8', 'x_ofs', 'host'): "the same index tables (host or device)",
    ('ops.pan_boundary_map', 'pred_2ch', 'strided'): "A non-contiguous map is copied",
    ('ops.pan_boundary_map', 'gt_rgb', 'strided'): "A non-contiguous map is copied",
    ('ops.mask_logit_gather', 'mask_logit', 'channels_last'): "any dense layout (NCHW or channels_last)",
    ('ops.mask_logit_gather', 'mask_logit', 'offset'): "it may start anywhere in an allocation (element-aligned)",
    ('ops.pyramid_proposals', 'cls_probs', 'offset'): "a channel slice of a wider map is read in place, wherever it starts",
    ('ops.pyramid_proposals', 'bbox_preds', 'offset'): "a channel slice of a wider map is read in place, wherever it starts",
    ('ops.restore_label_maps', 'sseg', 'offset'): "a crop may start at any element of the padded map",
    ('ops.restore_label_maps', 'pano', 'offset'): "a crop may start at any element of the padded map",
    ('ops.restore_plane_u8', 'plane', 'offset'): "a crop may start at any byte of the padded plane",
}

# abiguard.UNALIGNED parameter -> the wrapper argument that reaches it, whose `offset` row above is the run that confirms the reading
UNALIGNED_SLOT = {
    ('upsnet_mask_logit_gather', 'mask_logit'): ('ops.mask_logit_gather', 'mask_logit'),
    ('upsnet_pyramid_proposals_strided', 'cls_prob'): ('ops.pyramid_proposals', 'cls_probs'),         # (forwards to _strided_ordered,
    ('upsnet_pyramid_proposals_strided', 'bbox_pred'): ('ops.pyramid_proposals', 'bbox_preds'),       #  which the wrapper calls)
    ('upsnet_pyramid_proposals_strided_ordered', 'cls_prob'): ('ops.pyramid_proposals', 'cls_probs'),
    ('upsnet_pyramid_proposals_strided_ordered', 'bbox_pred'): ('ops.pyramid_proposals', 'bbox_preds'),
    ('upsnet_pyramid_proposals_joint_strided', 'cls_prob'): ('ops.pyramid_proposals', 'cls_probs'),
    ('upsnet_pyramid_proposals_joint_strided', 'bbox_pred'): ('ops.pyramid_proposals', 'bbox_preds'),
    ('upsnet_restore_label_maps', 'sseg'): ('ops.restore_label_maps', 'sseg'),
    ('upsnet_restore_label_maps', 'pano'): ('ops.restore_label_maps', 'pano'),
    ('upsnet_restore_plane_u8', 'src'): ('ops.restore_plane_u8', 'plane'),
}

_MODULES = {}


def _entry_modules():
    if not _MODULES:
        for m in abiguard.scan_package()[2]:
            _MODULES.setdefault(m.rsplit('.', 1)[-1], m)
    return _MODULES


def _owner(entry):
    mod, *path = entry.split('.')
    obj = importlib.import_module(_entry_modules()[mod])
    for p in path[:-1]:
        obj = getattr(obj, p)
    return obj, path[-1]


# ------------------------------------------------------------------------------------------------ a. canonical sweep
def _clone(obj):
    """Tensors cloned (layout and attached attributes kept), containers rebuilt, everything else by reference."""
    if isinstance(obj, torch.Tensor):
        c = obj.detach().clone()
        if obj.is_pinned():
            c = c.pin_memory()
        c.__dict__.update(obj.__dict__)
        return c
    if isinstance(obj, (list, tuple)):
        return type(obj)(_clone(o) for o in obj) if type(obj) in (list, tuple) else obj
    if isinstance(obj, dict):
        return {k: _clone(v) for k, v in obj.items()}
    return obj


_REF = {}


def _reference_kernels(tmod):
    if 'ref' not in _REF:
        _REF['ref'] = tmod.RefLib(tmod.VEC, os.path.join(tmod.ROOT, "oracle", "_ref", "libupsnet_ref.so"))
    return _REF['ref']


def run_canonical(case, capture=None):
    """The case's body under the guard. Returns (the Guard, [entry point] in call order). capture: {entry: None} -> filled with
    (function, args, kwargs) of the entry's first call, tensors cloned before the call."""
    calls = []
    tmod = importlib.import_module(case.module)
    if 'ref' in inspect.signature(getattr(tmod, case.test)).parameters:      # tests/test_backward_gpu.py's module fixture of that name
        case = case._replace(kwargs=dict(case.kwargs, ref=_reference_kernels(tmod)))
    with contextlib.ExitStack() as stack:
        mp = stack.enter_context(pytest.MonkeyPatch.context())
        fn, args = case_call(case, stack, mp)

        def counted(name, real):
            def wrapped(*a, **kw):
                calls.append(name)
                if capture is not None and name in capture and capture[name] is None:
                    capture[name] = (real, _clone(a), _clone(kw))
                return real(*a, **kw)
            wrapped.__wrapped__ = real
            return wrapped
        for e in case.entries:
            owner, name = _owner(e)
            real = getattr(owner, name)
            w = counted(e, real)
            if isinstance(inspect.getattr_static(owner, name), staticmethod):
                w = staticmethod(w)
            mp.setattr(owner, name, w)
        with abiguard.guard() as g:
            fn(**args, **case.kwargs)
            torch.cuda.synchronize()
    return g, calls


@pytest.mark.parametrize('case', ALL_CASES, ids=[c.id for c in ALL_CASES])
def test_canonical_forms_cross_the_abi_clean(case):
    g, calls = run_canonical(case)
    assert not g.violations, "\n".join(g.violations)
    assert set(calls) == set(case.entries), "entry points listed but never called: %s" % sorted(set(case.entries) - set(calls))


def odd_level_size():
    """The smallest padded size of tests/size_population.py at which some pyramid level (strides 4 .. 64) has an odd number of pixels:
    a map of 15, 18 or 27 channels at that level then ends off 16 bytes, and whatever is carved behind it starts there unless padded."""
    import size_population
    pairs = size_population.one_per_padded(size_population.coco_padded_sizes()) + size_population.cityscapes_sizes()
    odd = [p for _, p in pairs if any((-(-p[0] // s)) * (-(-p[1] // s)) % 2 for s in (4, 8, 16, 32, 64))]
    return min(odd, key=lambda p: (p[0] * p[1], p))


@pytest.mark.parametrize('preset,size', [('CITYSCAPES_R50', (256, 512)), ('COCO_R101_DCN', (256, 512)), ('COCO_R101_DCN', 'odd')],
                         ids=['CITYSCAPES_R50', 'COCO_R101_DCN', 'COCO_R101_DCN-odd-level'])
def test_eager_forward_crosses_the_abi_clean(preset, size):
    """'odd': odd_level_size(), 800 x 800 with 25 x 25 and 13 x 13 levels, on the preset with 15-channel RPN heads and 18 / 27-channel
    offset maps (padded blobs are multiples of 32, so the levels down to stride 16 are always even)."""
    cfg = importlib.import_module('upsnet_amd.config.config')
    height, width = odd_level_size() if size == 'odd' else size
    with sweep._saved_config():
        cfg.update_config_dict(getattr(cfg, preset))
        from upsnet_amd.synthetic import build_model, make_image
        model = build_model()
        data = make_image(height, width, seed=3, device='cuda')
        model.use_graph = False
        model._graphs.clear()
        with torch.no_grad(), abiguard.guard() as g:
            out = model(data)
            torch.cuda.synchronize()
        assert not g.violations, "\n".join(g.violations)
        assert g.launches() > 50 and 'panoptic_outputs' in out, g.launches()


# ------------------------------------------------------------------------------------------------ b. form sweep
def form_entries():
    """[(entry point, case)] of the form sweep: every module-level function among the cases' entries whose body calls the library with
    a pointer, with the first case that lists it (or the one FORM_CASE names)."""
    callers, _ = abiguard.pointer_callers()
    by_id = {c.id: c for c in ALL_CASES}
    seen = collections.OrderedDict()
    for c in ALL_CASES:
        for e in c.entries:
            if e in callers and e.count('.') == 1 and e not in seen:
                seen[e] = by_id[FORM_CASE[e]] if e in FORM_CASE else c
    return list(seen.items())


def form_excluded():
    callers, _ = abiguard.pointer_callers()
    return sorted({e for c in ALL_CASES for e in c.entries if e in callers and e.count('.') > 1})


DTYPE_VARIANT = {torch.float32: torch.float64, torch.int32: torch.int64, torch.int64: torch.int32, torch.bool: torch.uint8}


def strided_variant(t):
    """Equal values in a view that is contiguous in no memory format: the innermost dimension (of the physical layout) with more than
    one element comes ::2 out of a buffer twice as long. None where the tensor has at most one element."""
    if t.numel() <= 1:
        return None
    order = sorted(range(t.dim()), key=lambda d: (t.stride(d), -d), reverse=True)        # outermost .. innermost, physically
    inner = [d for d in order if t.shape[d] > 1][-1]
    phys = [t.shape[d] * (2 if d == inner else 1) for d in order]
    buf = torch.zeros(phys, dtype=t.dtype, device=t.device)
    inv = [order.index(d) for d in range(t.dim())]
    view = buf.permute(inv)
    index = [slice(None)] * t.dim()
    index[inner] = slice(None, None, 2)
    view = view[tuple(index)]
    view.copy_(t)
    assert view.shape == t.shape and not abiguard._some_memory_format(tuple(view.shape), tuple(view.stride()))
    view.__dict__.update(t.__dict__)
    return view


def offset_variant(t):
    """Equal values, sizes and strides (so memory format too) and the attached attributes, one element into a buffer one element longer:
    the address is a multiple of the element size and not of 16. None only where the tensor has no elements."""
    if t.numel() == 0:
        return None
    extent = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
    buf = torch.empty((extent + 1,), dtype=t.dtype, device=t.device)
    if t.is_pinned():
        buf = buf.pin_memory()
    assert buf.data_ptr() % 16 == 0 and t.element_size() < 16
    buf[1:].copy_(t.as_strided((extent,), (1,)))       # (the whole span t's strides reach, so an expanded or gapped view copies too)
    view = buf.as_strided(tuple(t.shape), tuple(t.stride()), 1)
    assert view.data_ptr() % 16 != 0 and view.shape == t.shape and view.stride() == t.stride()
    view.__dict__.update(t.__dict__)
    return view


def dtype_variant(t):
    if t.dtype not in DTYPE_VARIANT:
        return None
    v = t.to(DTYPE_VARIANT[t.dtype])
    v.__dict__.update(t.__dict__)
    return v


def rows_variant(t):
    """Equal values with the rows three elements further apart than they are long (columns stay contiguous)."""
    if t.dim() < 2 or t.numel() <= 1 or not t.is_contiguous():
        return None
    buf = torch.zeros(tuple(t.shape[:-1]) + (t.shape[-1] + 3,), dtype=t.dtype, device=t.device)
    view = buf[..., :t.shape[-1]]
    view.copy_(t)
    return view


def channels_last_variant(t):
    if t.dim() != 4 or t.is_contiguous(memory_format=torch.channels_last):
        return t.contiguous() if t.dim() == 4 and not t.is_contiguous() else None
    return t.contiguous(memory_format=torch.channels_last)


VARIANTS = (('strided', strided_variant), ('dtype', dtype_variant), ('offset', offset_variant))
PROMISED_VARIANTS = {'rows': rows_variant, 'host': lambda t: t.cpu() if t.is_cuda else None, 'channels_last': channels_last_variant}


def _slots(fn, args, kw):
    """[(argument name, path)] of every tensor among the arguments: path = (position or keyword,) + indices into lists / tuples."""
    params = [p.name for p in inspect.signature(fn).parameters.values()]
    out = []

    def walk(name, obj, path):
        if isinstance(obj, torch.Tensor):
            out.append((name, path))
        elif type(obj) in (list, tuple):
            for i, o in enumerate(obj):
                walk('%s[%d]' % (name, i), o, path + (i,))
    for i, a in enumerate(args):
        walk(params[i] if i < len(params) else 'arg%d' % i, a, (i,))
    for k, v in kw.items():
        walk(k, v, (k,))
    return out


def _get(args, kw, path):
    obj = kw[path[0]] if isinstance(path[0], str) else args[path[0]]
    for i in path[1:]:
        obj = obj[i]
    return obj


def _put(args, kw, path, value):
    def rebuilt(obj, rest):
        if not rest:
            return value
        items = list(obj)
        items[rest[0]] = rebuilt(obj[rest[0]], rest[1:])
        return type(obj)(items)
    args = list(args)
    if isinstance(path[0], str):
        kw = dict(kw)
        kw[path[0]] = rebuilt(kw[path[0]], path[1:])
    else:
        args[path[0]] = rebuilt(args[path[0]], path[1:])
    return tuple(args), kw


def _returned(entry, ret, args):
    region = sweep.DEFINED_REGION.get(entry)
    return [t.detach().clone() for t in sweep._tensors(region(ret, args) if region is not None else ret)]


def _values(t, like):
    """t's values in like's dtype, for the bitwise comparison of an argument that went in as a variant."""
    return t.to(device=like.device, dtype=like.dtype)


def _replay(entry, fn, args, kw, slots):
    """One call under a guard of its own: (outcome, detail, returned tensors, the arguments after the call)."""
    with abiguard.guard() as g:
        try:
            ret = fn(*args, **kw)
            torch.cuda.synchronize()
        except abiguard.AbiViolation as e:
            return 'violation', str(e), None, None
        except (ValueError, TypeError, RuntimeError) as e:
            torch.cuda.synchronize()
            if g.launches() == 0:
                return 'refused', '%s: %s' % (type(e).__name__, str(e)[:100]), None, None
            return 'failed after %d launches' % g.launches(), '%s: %s' % (type(e).__name__, e), None, None
        except Exception as e:          # (anything else is no refusal the sweep accepts)
            torch.cuda.synchronize()
            return 'raised %s' % type(e).__name__, str(e), None, None
    if g.violations:
        return 'violation', g.violations[0], None, None
    return 'ran', '', _returned(entry, ret, args), [_get(args, kw, p) for _, p in slots]


def form_outcomes(entry, case):
    """[(entry, argument, variant, outcome, detail)] for every tensor argument of the entry's first call in `case`."""
    capture = {entry: None}
    try:
        run_canonical(case, capture)
    except Exception:       # (the body's own trouble is the canonical sweep's to report; here only the entry's first call is wanted)
        if capture[entry] is None:
            raise
    assert capture[entry] is not None, "%s was not called by %s" % (entry, case.id)
    fn, args0, kw0 = capture[entry]
    slots = _slots(fn, args0, kw0)
    before0 = [_get(args0, kw0, p).clone() for _, p in slots]
    runs = []
    for _ in range(2):      # twice: what two canonical replays do not reproduce (float atomics, scratch) is not compared
        out, detail, ret, after = _replay(entry, fn, _clone(args0), _clone(kw0), slots)
        if out != 'ran':        # the canonical form itself does not cross clean: one row says so, no variant is tried
            return [(entry, '(as the case calls it)', 'canonical', out, detail)]
        runs.append((ret, after))
    (ret0, after0), (ret1, after1) = runs
    assert len(ret0) == len(ret1)
    stable_ret = [memguard.bit_equal(a, b) for a, b in zip(ret0, ret1)]
    # (a workspace is scratch: hash slots and lists taken with atomics, in an order that differs from run to run even where two
    # replays happen to agree. What it must hold afterwards -- zeros -- is the poisoned sweep's and the feature tests' to check.)
    # Every other tensor argument is compared after the call, written or not: an accumulator that the kernel rewrites with the values
    # it already held must still hold them under a variant.
    compared = ['workspace' not in name for name, _ in slots]
    stable_arg = [memguard.bit_equal(a, b) for a, b in zip(after0, after1)]
    untouched = [memguard.bit_equal(a, b) for a, b in zip(before0, after0)]
    rows = []
    for k, (name, path) in enumerate(slots):
        base = name.split('[')[0]
        for vname, make in VARIANTS + tuple((v, PROMISED_VARIANTS[v]) for (e, a, v) in PROMISED if (e, a) == (entry, base) and v in PROMISED_VARIANTS):
            args, kw = _clone(args0), _clone(kw0)
            v = make(_get(args, kw, path))
            if v is None:
                continue
            args, kw = _put(args, kw, path, v)
            v_before = v.clone()
            out, detail, ret, after = _replay(entry, fn, args, kw, slots)
            if out == 'ran':
                diff = [i for i, (a, b) in enumerate(zip(ret0, ret)) if stable_ret[i] and not memguard.bit_equal(a, b)]
                if len(ret) != len(ret0):
                    diff = ['count']
                # the replaced argument, where the canonical replay leaves it as it was, must be as it went in (in its own dtype: the
                # unspecified rows of a capacity-sized int64 input need not survive a trip through int32); every other one, and a
                # replaced one that is written, must hold what the canonical replay left
                darg = [slots[i][0] for i in range(len(slots)) if compared[i] and stable_arg[i]
                        and not (memguard.bit_equal(v_before, after[i]) if i == k and untouched[i]
                                 else memguard.bit_equal(after0[i], _values(after[i], after0[i])))]
                out = 'same' if not diff and not darg else 'different'
                detail = 'returned %s, arguments %s' % (diff, darg) if out == 'different' else ''
            rows.append((entry, name, vname, out, detail))
    return rows


_FORMS = form_entries()


@pytest.mark.parametrize('entry,case', _FORMS, ids=[e for e, _ in _FORMS])
def test_every_argument_form_is_taken_or_refused(entry, case):
    rows = form_outcomes(entry, case)       # (none where the entry takes no tensor: host arrays, lists of numpy arrays)
    for r in rows:
        print("%s %s %s: %s %s" % r)
    if os.environ.get('UPSNET_ABI_FORMS_JSON'):       # (tools/abi_forms.py merges two such files into profiles/abi_forms.txt)
        import json
        with open(os.environ['UPSNET_ABI_FORMS_JSON'], 'a') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')
    bad = [r for r in rows if r[3] not in ('same', 'refused')]
    assert not bad, "\n".join("%s(%s) as %s: %s -- %s" % r for r in bad)
    got = {(r[0], r[1].split('[')[0], r[2]): r[3] for r in rows}
    for key in [k for k in PROMISED if k[0] == entry]:          # every promise, not one per entry: replayed, and `same`
        assert key in got, "the promised form %s was not replayed: the captured call hands no tensor for it" % (key,)
        assert got[key] == 'same', "the docstring promises %r, but %s came out %s" % (PROMISED[key], key, got[key])


def test_promised_forms_are_swept():
    """Every promise names an argument of an entry the form sweep replays (a renamed argument would drop out silently)."""
    entries = dict(_FORMS)
    for (entry, arg, variant), why in PROMISED.items():
        assert entry in entries, entry
        owner, name = _owner(entry)
        assert arg in inspect.signature(getattr(owner, name)).parameters, (entry, arg)
        assert (variant in dict(VARIANTS) or variant in PROMISED_VARIANTS) and len(why) > 10
