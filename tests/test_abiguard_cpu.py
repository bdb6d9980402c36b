"""CPU: the three copies of every C-ABI signature agree (include/upsnet_hip.h, the extern "C" definitions in upsnet_amd/csrc, the
argtypes rows of upsnet_amd/_lib.py); tests/abiguard.py detects what it claims, on a stub library and host tensors; the guard patches
every module that holds ptr / ptr_array / lib; no address leaves a tensor outside _lib.py; and every function of the package that hands a
pointer to the library is an entry of a case of tests/test_abi_contract_gpu.py (or excluded with a reason)."""
import ast
import collections
import ctypes
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abiguard  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the three copies of a signature
def test_header_abi_reads_types_names_and_arrays():
    h = abiguard.header_abi()
    assert len(h) >= 195
    assert h['upsnet_last_error'] == ('char*', [])
    assert h['upsnet_zero_fill'] == ('int', [('stream', 'void*'), ('ptr', 'void*'), ('bytes', 'size_t')])
    assert h['upsnet_roi_tuning'] == ('void', [('variant', 'int')])
    fpn = dict(h['upsnet_fpn_roi_align_forward'][1])
    assert fpn['feat_nhwc'] == 'float**' and fpn['feat_h'] == 'int*' and fpn['spatial_scale'] == 'float*' and fpn['channels'] == 'int'
    gather = h['upsnet_mask_logit_gather'][1]
    assert gather[5:10] == [('stride_n', 'long'), ('stride_c', 'long'), ('stride_e', 'long'), ('row', 'int*'), ('cls', 'long*')]
    assert dict(h['upsnet_cs_inst_image'][1])['gt_t'] == 'unsigned short*'          # (a parameter NAME that ends in _t)
    assert dict(h['upsnet_mask_roi'][1])['reg_weights_host'] == 'float*'            # (const float w[4] is a pointer)
    every = {t for _, ps in h.values() for _, t in ps} | {r for r, _ in h.values()}
    assert every <= {'char*', 'double', 'double*', 'float', 'float*', 'float**', 'int', 'int*', 'int**', 'long', 'long*', 'size_t', 'size_t*',
                     'unsigned char*', 'unsigned char**', 'unsigned short*', 'unsigned*', 'void', 'void*', 'void**'}, sorted(every)
    assert all(n for _, ps in h.values() for n, _ in ps), "a parameter without a name"
    assert all(t.rstrip('*') in abiguard.ELEMENT_DTYPES for _, ps in h.values() for _, t in ps if t.endswith('*')), "an element type without a rule"


def test_the_three_copies_of_every_signature_agree():
    header, defs, binding = abiguard.header_abi(), abiguard.definition_abi(), abiguard.binding_abi()
    assert set(header) == set(defs) == set(binding)
    bad = abiguard.signature_mismatches(header, defs, binding)
    assert not bad, "\n".join(bad)


def test_signature_mismatches_name_symbol_and_parameter(tmp_path):
    """The comparison has teeth: a c_double bound as c_float, an int dropped from a declaration, a second definition, a changed
    pointer element type and a changed result are each reported with the symbol and the parameter."""
    from upsnet_amd import _lib
    header, defs, binding = abiguard.header_abi(), abiguard.definition_abi(), abiguard.binding_abi()
    sigs = dict(_lib._SIGNATURES)
    res, args = sigs['upsnet_mask_removal']
    k = args.index(ctypes.c_double)
    sigs['upsnet_mask_removal'] = (res, args[:k] + [ctypes.c_float] + args[k + 1:])
    bad = abiguard.signature_mismatches(header, defs, abiguard.binding_abi(sigs))
    assert len(bad) == 1 and 'upsnet_mask_removal' in bad[0] and 'fraction_threshold' in bad[0] and 'c_float' in bad[0], bad

    text = open(os.path.join(ROOT, abiguard.HEADER)).read()
    cut = text.replace("int upsnet_mask_paste(void *stream, const float *mask_rois, const float *mask_logit, const int64_t *keep_inds,",
                       "int upsnet_mask_paste(void *stream, const float *mask_rois, const float *mask_logit, const int *keep_inds,")
    assert cut != text
    p = tmp_path / 'h.h'
    p.write_text(cut)
    bad = abiguard.signature_mismatches(abiguard.header_abi(str(p)), defs, binding)
    assert len(bad) == 1 and 'upsnet_mask_paste' in bad[0] and 'keep_inds' in bad[0] and 'long*' in bad[0], bad

    ret, params = header['upsnet_seg_term']
    k = [i for i, (n, t) in enumerate(params) if t == 'int'][0]
    dropped = dict(header)
    dropped['upsnet_seg_term'] = (ret, params[:k] + params[k + 1:])
    bad = abiguard.signature_mismatches(dropped, defs, binding)
    assert len(bad) == 4 and all('upsnet_seg_term' in b for b in bad), bad          # arity and first shifted type, in both other copies
    first = next(i for i in range(k, len(params) - 1) if params[i][1] != params[i + 1][1])      # (three ints in a row: the first shifted TYPE)
    assert any('has %d parameters' % (len(params) - 1) in b for b in bad)
    assert sum('parameter %d (%s)' % (first, params[first + 1][0]) in b for b in bad) == 2, bad

    twice = dict(defs)
    twice['upsnet_abi_version'] = defs['upsnet_abi_version'] * 2
    bad = abiguard.signature_mismatches(header, twice, binding)
    assert len(bad) == 1 and 'upsnet_abi_version: 2 definitions' in bad[0], bad
    other = dict(header)
    other['upsnet_abi_version'] = ('long', [])
    bad = abiguard.signature_mismatches(other, defs, binding)
    assert len(bad) == 2 and all('upsnet_abi_version: result' in b for b in bad), bad


# ------------------------------------------------------------------------------------------------ the guard on a stub library
class Stub:
    """Stands in for the loaded library: every upsnet_* attribute is a function that counts its calls."""

    def __init__(self):
        self.calls = collections.Counter()

    def __getattr__(self, name):
        if not name.startswith('upsnet_'):
            raise AttributeError(name)

        def fn(*args):
            self.calls[name] += 1
            return 0
        return fn


def _gather(lib, ptr, logits, row, cls, out, stream=None):
    n, C, h, w = logits.shape
    return lib().upsnet_mask_logit_gather(stream, ptr(logits), n, C, h * w, logits.stride(0), logits.stride(1), logits.stride(3), ptr(row),
                                          ptr(cls), row.shape[0], ptr(out))


KEEP = {}      # holds the mistyped / strided tensors of a violating call alive, so that the rule under test is the one that fires


def _tensors():
    return (torch.zeros(3, 4, 2, 2), torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int64), torch.zeros(5, 1, 2, 2))


def test_a_clean_call_goes_through_exactly_once():
    from upsnet_amd import _lib
    stub = Stub()
    logits, row, cls, out = _tensors()
    with abiguard.guard(library=stub) as g:
        assert _gather(_lib.lib, _lib.ptr, logits, row, cls, out) == 0
        p = _lib.ptr(row)
        assert isinstance(p, ctypes.c_void_p) and p.value == row.data_ptr() and _lib.ptr(None) is None
        a = _lib.ptr_array([row, None, cls])
        assert [a[0], a[1], a[2]] == [row.data_ptr(), None, cls.data_ptr()]
        assert _lib.addr(out) == out.data_ptr()
        assert _lib.lib().upsnet_nms_workspace_bytes(2, 3) == 0       # (no pointer parameter: counted, but no launch)
    assert stub.calls == {'upsnet_mask_logit_gather': 1, 'upsnet_nms_workspace_bytes': 1}
    assert g.calls == stub.calls and g.launches() == 1 and not g.violations


def _refused(call, rule, *names):
    stub = Stub()
    with abiguard.guard(library=stub) as g:
        with pytest.raises(abiguard.AbiViolation) as e:
            call()
    msg = str(e.value)
    assert not stub.calls and g.launches() == 0, "a refused call reached the library"
    assert rule in msg and os.path.basename(__file__) in msg and g.violations == [msg], msg
    for n in names:
        assert n in msg, (n, msg)
    return msg


def test_origin_rule():
    from upsnet_amd import _lib
    logits, row, cls, out = _tensors()
    bare = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731  (an address that did not come out of ptr())
    stub = Stub()
    with abiguard.guard(library=stub) as g:
        with pytest.raises(abiguard.AbiViolation) as e:
            _lib.lib().upsnet_mask_logit_gather(None, _lib.ptr(logits), 3, 4, 4, 16, 4, 1, bare(row), _lib.ptr(cls), 5, _lib.ptr(out))
    assert not stub.calls and 'origin' in str(e.value) and 'upsnet_mask_logit_gather(row)' in str(e.value), str(e.value)
    # a host array of bare addresses where the header wants an array of pointers
    feats = [torch.zeros(1, 2, 2, 4) for _ in range(4)]
    rois, out4 = torch.zeros(1, 5), torch.zeros(1, 7, 7, 4)
    arr = (ctypes.c_void_p * 4)(*[f.data_ptr() for f in feats])
    four = _lib.int_array([2] * 4)
    with abiguard.guard(library=stub) as g:
        with pytest.raises(abiguard.AbiViolation) as e:
            _lib.lib().upsnet_fpn_roi_align_forward(None, arr, four, four, _lib.float_array([1.] * 4), 4, _lib.ptr(rois), 1, None, 7, 7, 2,
                                                    _lib.ptr(out4), None)
        assert 'origin' in str(e.value) and 'feat_nhwc[0]' in str(e.value)
        # ... and the same call with ptr_array, host int / float arrays and NULLs is clean; `stream` may be anything
        assert _lib.lib().upsnet_fpn_roi_align_forward(ctypes.c_void_p(12345), _lib.ptr_array(feats), four, four, _lib.float_array([1.] * 4), 4,
                                                       _lib.ptr(rois), 1, None, 7, 7, 2, _lib.ptr(out4), None) == 0
    assert stub.calls == {'upsnet_fpn_roi_align_forward': 1} and g.launches() == 1


def test_liveness_rule_on_the_two_temporaries_of_one_argument_list():
    """The pattern mask_logit_gather had: ptr(row.to(int32).contiguous()), ptr(cls.to(int64).contiguous()) in one argument list, with
    row and cls of other dtypes, so that both conversions are temporaries that die when ptr() returns."""
    from upsnet_amd import _lib
    logits, _, _, out = _tensors()
    row, cls = torch.zeros(5, dtype=torch.int64), torch.zeros(5, dtype=torch.int32)

    def call():
        _lib.lib().upsnet_mask_logit_gather(None, _lib.ptr(logits), 3, 4, 4, 16, 4, 1, _lib.ptr(row.to(torch.int32).contiguous()),
                                            _lib.ptr(cls.to(torch.int64).contiguous()), 5, _lib.ptr(out))
    msg = _refused(call, 'liveness', 'upsnet_mask_logit_gather(row)', 'freed before launch', 'call')
    assert 'int32' in msg
    # bound to locals first, the same conversions are fine; so is a view whose base lives
    stub = Stub()
    with abiguard.guard(library=stub) as g:
        r, c = row.to(torch.int32).contiguous(), cls.to(torch.int64).contiguous()
        _gather(_lib.lib, _lib.ptr, logits, r, c, out)
        big = torch.zeros(9, dtype=torch.int32)
        _lib.lib().upsnet_mask_logit_gather(None, _lib.ptr(logits), 3, 4, 4, 16, 4, 1, _lib.ptr(big[4:]), _lib.ptr(c), 5, _lib.ptr(out))
    assert g.launches() == 2 and not g.violations
    # ... but not a view of a temporary
    _refused(lambda: _lib.lib().upsnet_mask_logit_gather(None, _lib.ptr(logits), 3, 4, 4, 16, 4, 1, _lib.ptr(row.to(torch.int32)[0:]),
                                                         _lib.ptr(c), 5, _lib.ptr(out)), 'liveness', '(row)')
    # ... and an element of ptr_array that died
    parts = [logits.clone(), logits]
    _refused(lambda: _lib.lib().upsnet_fcn_score_combine(None, 2, _lib.ptr_array([logits.clone(), logits]), 4, 2, 2, None, _lib.ptr(out)),
             'liveness', 'upsnet_fcn_score_combine(part[0])')
    with abiguard.guard(library=Stub()) as g:
        _lib.lib().upsnet_fcn_score_combine(None, 2, _lib.ptr_array(parts), 4, 2, 2, None, _lib.ptr(out))
    assert g.launches() == 1


def test_element_type_rule():
    from upsnet_amd import _lib
    logits, row, cls, out = _tensors()
    _refused(lambda: _gather(_lib.lib, _lib.ptr, logits, row, KEEP.setdefault('c', cls.int()), out), 'element type', 'upsnet_mask_logit_gather(cls)', 'torch.int32', 'long')
    _refused(lambda: _gather(_lib.lib, _lib.ptr, KEEP.setdefault('l', logits.double()), row, cls, out), 'element type', '(mask_logit)', 'float64')
    # void * takes anything; unsigned char takes uint8 / int8 / bool; the 16-bit types take bfloat16 / float16 / int16
    stub = Stub()
    u8, b, i16, bf = torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.bool), torch.zeros(4, dtype=torch.int16), torch.zeros(4, dtype=torch.bfloat16)
    with abiguard.guard(library=stub) as g:
        for t in (u8, b, i16, bf, logits):
            _lib.lib().upsnet_zero_fill(None, _lib.ptr(t), 4)
        for t in (u8, b, u8.view(torch.int8)):
            KEEP['v'] = t
            _lib.lib().upsnet_vis_font(_lib.ptr(t))
    assert g.launches() == 8
    h = abiguard.header_abi()
    sym, pname = next((s, n) for s, (_, ps) in h.items() for n, t in ps if t == 'unsigned short*')
    args = [None] * len(h[sym][1])
    k = [n for n, _ in h[sym][1]].index(pname)
    for t, ok in ((i16, True), (bf, True), (bf.to(torch.float16), True), (u8, False), (logits, False)):
        KEEP['h'] = t
        with abiguard.guard(library=stub) as g:
            args[k] = _lib.ptr(t)
            if ok:
                getattr(_lib.lib(), sym)(*args)
            else:
                with pytest.raises(abiguard.AbiViolation, match='element type'):
                    getattr(_lib.lib(), sym)(*args)


def test_density_rule_and_the_strided_table():
    from upsnet_amd import _lib
    logits, row, cls, out = _tensors()
    wide = torch.zeros(10, dtype=torch.int32)
    KEEP['r'] = wide[::2]
    _refused(lambda: _gather(_lib.lib, _lib.ptr, logits, KEEP['r'], cls, out), 'density', 'upsnet_mask_logit_gather(row)', '(2,)')
    stub = Stub()
    sliced = torch.zeros(3, 8, 2, 2)[:, ::2]                       # contiguous in no memory format
    assert not sliced.is_contiguous() and not sliced.is_contiguous(memory_format=torch.channels_last)
    with abiguard.guard(library=stub) as g:
        _gather(_lib.lib, _lib.ptr, sliced, row, cls, out)          # listed: the entry point takes the three strides
        _gather(_lib.lib, _lib.ptr, logits.contiguous(memory_format=torch.channels_last), row, cls, out)
        _gather(_lib.lib, _lib.ptr, logits, row[:1], cls, out)      # one element: nothing to stride over
    assert g.launches() == 3
    with abiguard.guard(library=stub, strided={}) as g:
        with pytest.raises(abiguard.AbiViolation, match='density'):
            _gather(_lib.lib, _lib.ptr, sliced, row, cls, out)
    h = abiguard.header_abi()
    for (sym, pname), why in abiguard.STRIDED.items():
        params = dict(h[sym][1])
        assert params[pname].endswith('*') and len(why) > 20
        assert any(n in why for n, t in h[sym][1] if 'stride' in n), "%s(%s): the reason names no stride parameter" % (sym, pname)
    for (sym, pname), why in abiguard.HOST.items():
        assert dict(h[sym][1])[pname].endswith('*') and len(why) > 20


def test_device_rule(monkeypatch):
    """Needs no second GPU: the rule is a comparison of the recorded device with the current one."""
    from upsnet_amd import _lib
    logits, row, cls, out = _tensors()
    real = abiguard._record

    def on_cuda1(t, site):
        r = real(t, site)
        return r._replace(device=torch.device('cuda', 1)) if t is row else r
    monkeypatch.setattr(abiguard, '_record', on_cuda1)
    monkeypatch.setattr(abiguard, '_current_device', lambda: 0)
    _refused(lambda: _gather(_lib.lib, _lib.ptr, logits, row, cls, out), 'device', 'upsnet_mask_logit_gather(row)', 'cuda:1', 'cuda:0')
    monkeypatch.setattr(abiguard, '_current_device', lambda: 1)
    stub = Stub()
    with abiguard.guard(library=stub) as g:
        _gather(_lib.lib, _lib.ptr, logits, row, cls, out)
    assert g.launches() == 1


def test_argument_count_is_checked_against_the_header():
    from upsnet_amd import _lib
    with abiguard.guard(library=Stub()):
        with pytest.raises(TypeError, match='upsnet_zero_fill takes 3'):
            _lib.lib().upsnet_zero_fill(None, None)


# ------------------------------------------------------------------------------------------------ what the guard patches
def test_every_module_that_holds_a_pointer_maker_is_patched_and_restored():
    found = abiguard.holders()
    assert len(found) >= 18 and {'upsnet_amd._lib', 'upsnet_amd.ops', 'upsnet_amd.tta', 'upsnet_amd.group_norm', 'upsnet_amd.dataset.coco_eval',
                                 'upsnet_amd.dataset.pan_track', 'upsnet_amd.models.resnet_upsnet'} <= set(found)
    lib_mod = importlib.import_module('upsnet_amd._lib')
    mods = {m: importlib.import_module(m) for m in found}
    real = {n: getattr(lib_mod, n) for n in abiguard.PATCHED}
    for m, names in found.items():          # the scan and the modules agree: what is imported by name is the real function
        for n in names:
            assert mods[m].__dict__[n] is real[n], (m, n)
    # nothing else in the package holds one of them under any name
    for name, m in list(sys.modules.items()):
        if name.startswith('upsnet_amd') and m is not None:
            for k, v in m.__dict__.items():
                if any(v is r for r in real.values()):
                    assert name in found and k in found[name], "%s.%s holds a pointer maker that the scan does not see" % (name, k)
    for raising in (False, True):
        try:
            with abiguard.guard(library=Stub()):
                for m, names in found.items():
                    for n in names:
                        assert mods[m].__dict__[n] is not real[n], "%s.%s is not patched" % (m, n)
                        assert mods[m].__dict__[n] is lib_mod.__dict__[n], "%s.%s is not the guard's" % (m, n)
                if raising:
                    raise ZeroDivisionError
        except ZeroDivisionError:
            assert raising
        for m, names in found.items():
            for n in names:
                assert mods[m].__dict__[n] is real[n], "%s.%s was not restored" % (m, n)


# ------------------------------------------------------------------------------------------------ one choke point for addresses
# .data_ptr() outside _lib.py: (file, function) -> why it is no address handed to the library
DATA_PTR_ALLOWED = {
    ('upsnet_amd/ops.py', 'cached_pack'): "part of the cache key of a packed weight (with the tensor's version): compared, never dereferenced",
    ('upsnet_amd/ops.py', 'pan_track_step_motion'): "alignment check (% 16) of the motion workspace before it goes through ptr()",
    ('upsnet_amd/ops.py', '_pan_clean'): "alignment checks (% 16) of labels and workspace before they go through ptr()",
    ('upsnet_amd/ops.py', 'pan_segment_scores'): "alignment check (% 4) of the workspace before it goes through ptr()",
}


def test_no_address_leaves_a_tensor_outside_the_binding():
    sites = abiguard.scan_package()[3]
    seen = set()
    for rel, line, fn, src in sites:
        key = (rel.replace(os.sep, '/'), fn)
        assert key in DATA_PTR_ALLOWED, "%s:%d (%s): .data_ptr() outside _lib.py -- use ptr / ptr_array / addr: %s" % (rel, line, fn, src)
        if 'cached_pack' not in fn:
            assert '%' in src, "%s:%d: allowed as an alignment check, but the line takes no remainder: %s" % (rel, line, src)
        seen.add(key)
    assert seen == set(DATA_PTR_ALLOWED), "allowed sites that no longer exist: %s" % sorted(set(DATA_PTR_ALLOWED) - seen)
    assert all(len(r) > 20 for r in DATA_PTR_ALLOWED.values())


def test_no_pointer_is_taken_of_an_expression_s_temporary():
    """ptr(f(x)) hands out the address of a tensor that nothing holds once ptr() returns. Statically: the argument of ptr() is a name,
    an attribute, a subscript (an element of a list or dict that holds it, or a view whose base lives) or None; ptr_array's a name, or a
    list built in place of such."""
    def plain(a):
        if isinstance(a, ast.IfExp):
            return plain(a.body) and plain(a.orelse)
        if isinstance(a, ast.Subscript):
            return plain(a.value)
        return isinstance(a, (ast.Name, ast.Attribute)) or (isinstance(a, ast.Constant) and a.value is None)
    bad = []
    for path, rel, mod in abiguard._package_files():
        tree = ast.parse(open(path).read(), rel)
        for n in ast.walk(tree):
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in ('ptr', 'ptr_array') and n.args:
                a = n.args[0]
                if n.func.id == 'ptr_array' and isinstance(a, ast.Call) and isinstance(a.func, ast.Name) and a.func.id == 'list' and plain(a.args[0]):
                    continue
                if n.func.id == 'ptr_array' and isinstance(a, ast.BinOp):          # [None] * A
                    continue
                if not plain(a):
                    bad.append("%s:%d: %s(%s)" % (rel, n.lineno, n.func.id, ast.unparse(a)))
    assert not bad, "pointers of temporaries (bind the tensor to a local first): %s" % "; ".join(bad)


# ------------------------------------------------------------------------------------------------ coverage of the sweep tables
def test_every_function_that_hands_a_pointer_to_the_library_has_a_case():
    import test_abi_contract_gpu as contract
    found, every = abiguard.pointer_callers()
    assert len(found) >= 105, sorted(found)
    covered = set()
    for c in contract.ALL_CASES:
        covered.update(c.entries)
    excluded = dict(contract.EXCLUDED)
    assert all(isinstance(r, str) and len(r) > 20 for r in excluded.values())
    missing = sorted(found - covered - set(excluded))
    assert not missing, "functions that call the library with a pointer, with no case and no reasoned exclusion: %s" % missing
    assert not set(excluded) - found, "excluded functions that hand no pointer to the library (or do not exist): %s" % sorted(set(excluded) - found)
    assert not covered - every, "the case tables name functions that do not exist (renamed?): %s" % sorted(covered - every)
    assert not covered & set(excluded), sorted(covered & set(excluded))
    assert len({c.id for c in contract.ALL_CASES}) == len(contract.ALL_CASES), "two cases share an id"
    # the form sweep: every module-level wrapper is replayed; only methods of stateful objects are left out
    forms = {e for e, _ in contract.form_entries()}
    assert forms == {e for e in found & covered if e.count('.') == 1}
    assert set(contract.form_excluded()) == {e for e in found & covered if e.count('.') > 1}
    assert len(contract.FORM_EXCLUDED_REASON) > 20
    for e in contract.form_excluded():       # each is a method of a class of the package
        mod, cls, meth = e.split('.')
        assert e in every and cls[0].isupper(), e
