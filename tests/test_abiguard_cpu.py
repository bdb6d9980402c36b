"""CPU: the three copies of every C-ABI signature agree (include/upsnet_hip.h, the extern "C" definitions in upsnet_amd/csrc, the
argtypes rows of upsnet_amd/_lib.py); tests/abiguard.py detects what it claims, on a stub library and host tensors (the alignment rule
and its UNALIGNED table included, with the binding's normalisers and refusals and the sweep's offset variant); the guard patches
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


def test_alignment_rule_and_the_unaligned_table():
    """Host tensors stand in for device ones: the rule is a remainder of the recorded address. The binding's own refusal (_lib.ptr) is
    opted out of here, so that the guard's rule is the one under test; the binding's is tested below."""
    from upsnet_amd import _lib
    logits, row, cls, out = _tensors()
    far = lambda t: _lib.ptr(t, unaligned=True)       # noqa: E731
    off_row = torch.zeros(6, dtype=torch.int32)[1:]
    off_cls = torch.zeros(6, dtype=torch.int64)[1:]
    off_out = torch.zeros(21)[1:].view(5, 1, 2, 2)
    off_logits = torch.zeros(49)[1:].view(3, 4, 2, 2)
    assert all(t.data_ptr() % 16 for t in (off_row, off_cls, off_out, off_logits)) and row.data_ptr() % 16 == 0
    msg = _refused(lambda: _gather(_lib.lib, far, logits, off_row, cls, out), 'alignment', 'upsnet_mask_logit_gather(row)', '4 bytes past')
    assert 'int32' in msg and 'UNALIGNED' in msg
    _refused(lambda: _gather(_lib.lib, far, logits, row, off_cls, out), 'alignment', 'upsnet_mask_logit_gather(cls)', '8 bytes past')
    _refused(lambda: _gather(_lib.lib, far, logits, row, cls, off_out), 'alignment', 'upsnet_mask_logit_gather(out)')
    stub = Stub()
    with abiguard.guard(library=stub) as g:
        _gather(_lib.lib, far, logits, row, cls, out)                 # aligned: passes
        _gather(_lib.lib, far, off_logits, row, cls, out)             # listed in UNALIGNED: passes
        _gather(_lib.lib, far, logits, torch.zeros(9, dtype=torch.int32)[4:], cls, out)       # 16 bytes into a buffer: aligned
    assert g.launches() == 3 and not g.violations
    with abiguard.guard(library=Stub(), unaligned={}) as g:
        with pytest.raises(abiguard.AbiViolation, match='alignment'):
            _gather(_lib.lib, far, off_logits, row, cls, out)
    # every element of a ptr_array, named with its index, and a NULL element passes
    parts = [logits, off_logits]
    msg = _refused(lambda: _lib.lib().upsnet_fcn_score_combine(None, 2, _lib.ptr_array(parts, unaligned=True), 4, 2, 2, None, _lib.ptr(out)),
                   'alignment', 'upsnet_fcn_score_combine(part[1])')
    with abiguard.guard(library=Stub()) as g:
        _lib.lib().upsnet_fcn_score_combine(None, 2, _lib.ptr_array([logits, None]), 4, 2, 2, None, _lib.ptr(out))
    assert g.launches() == 1
    # ... and of a ptr_array of an UNALIGNED parameter: the key is the parameter, not the element
    h = abiguard.header_abi()
    sym = 'upsnet_pyramid_proposals_joint_strided'
    args = [None] * len(h[sym][1])
    names = [n for n, _ in h[sym][1]]
    with abiguard.guard(library=Stub()) as g:
        args[names.index('cls_prob')] = _lib.ptr_array([off_logits, logits], unaligned=True)
        getattr(_lib.lib(), sym)(*args)
    assert g.launches() == 1 and not g.violations
    # an address recorded through addr(): a table of bare addresses where the header wants an array of pointers
    feats = [torch.zeros(17)[1:].view(1, 2, 2, 4)] + [torch.zeros(1, 2, 2, 4) for _ in range(3)]
    rois, out4 = torch.zeros(1, 5), torch.zeros(1, 7, 7, 4)
    four = _lib.int_array([2] * 4)

    def by_address():
        arr = (ctypes.c_void_p * 4)(*[_lib.addr(f, unaligned=True) for f in feats])
        _lib.lib().upsnet_fpn_roi_align_forward(None, arr, four, four, _lib.float_array([1.] * 4), 4, _lib.ptr(rois), 1, None, 7, 7, 2,
                                                _lib.ptr(out4), None)
    _refused(by_address, 'alignment', 'upsnet_fpn_roi_align_forward(feat_nhwc[0])')


def test_the_unaligned_table_is_well_formed():
    import test_abi_contract_gpu as contract
    h = abiguard.header_abi()
    _, callers, _, _ = abiguard.scan_package()
    calls = {m.rsplit('.', 1)[-1] + '.' + q: syms for m, fs in callers.items() for q, syms in fs.items()}
    assert abiguard.ALIGN == 16 and abiguard.UNALIGNED
    assert set(contract.UNALIGNED_SLOT) == set(abiguard.UNALIGNED)
    for (sym, pname), why in abiguard.UNALIGNED.items():
        assert sym in h, sym
        params = dict(h[sym][1])
        assert pname in params and params[pname].endswith('*') and pname != 'stream', (sym, pname)
        assert 'workspace' not in pname and not pname.endswith('_host') and (sym, pname) not in abiguard.HOST, (sym, pname)
        assert len(why) > 40 and len(why.split()) > 8 and '.hip' in why, "%s(%s): the justification names no kernel file" % (sym, pname)
        entry, arg = contract.UNALIGNED_SLOT[(sym, pname)]
        assert (entry, arg, 'offset') in contract.PROMISED, "%s(%s) has no PROMISED offset row" % (sym, pname)
        # the wrapper of the row reaches the symbol: it calls it, or an entry point whose definition forwards to it
        reached = calls[entry]
        assert sym in reached or any(s.startswith(sym) for s in reached), (entry, sym, sorted(reached))
    # and every promised offset row belongs to an UNALIGNED parameter
    for (entry, arg, variant) in contract.PROMISED:
        if variant == 'offset':
            assert (entry, arg) in set(contract.UNALIGNED_SLOT.values()), (entry, arg)


def test_the_binding_normalises_reads_and_refuses_writes_off_alignment():
    from upsnet_amd import _lib
    base32, base64 = torch.arange(9, dtype=torch.float32), torch.arange(9, dtype=torch.int64)
    cases = ((_lib.f32c, base32), (_lib.i32c, base32.to(torch.int32)), (_lib.i64c, base64), (_lib.dense, base32.to(torch.bfloat16)),
             (_lib.dense, base32.to(torch.uint8)), (_lib.aligned, base64))
    for fn, t in cases:
        assert t.data_ptr() % 16 == 0 and fn(t) is t, fn.__name__                 # aligned and in form: the same object
        off = t[1:]
        off.tag = 'kept'
        got = fn(off)
        assert off.data_ptr() % 16 and got is not off and got.data_ptr() % 16 == 0, fn.__name__
        assert got.dtype == off.dtype and torch.equal(got, off) and got.is_contiguous() and got.tag == 'kept'
        assert torch.equal(t, torch.arange(9).to(t.dtype)), "the input was modified"
    assert _lib.f32c(None) is None and _lib.dense(None) is None and _lib.aligned(None) is None
    assert _lib.f32c(base64[1:]).data_ptr() % 16 == 0 and _lib.f32c(base64[1:]).dtype == torch.float32       # converted: a fresh block
    # nhwc: channels_last kept, values equal, aligned; an aligned channels_last tensor is the same object
    x = torch.arange(2 * 3 * 2 * 2, dtype=torch.float32).view(2, 3, 2, 2).contiguous(memory_format=torch.channels_last)
    assert _lib.nhwc(x) is x
    buf = torch.zeros(x.numel() + 1)
    off = buf.as_strided(tuple(x.shape), tuple(x.stride()), 1)
    off.copy_(x)
    got = _lib.nhwc(off)
    assert off.data_ptr() % 16 and got.data_ptr() % 16 == 0 and torch.equal(got, x) and got.stride() == x.stride()
    # written: taken as it is, or refused with the word
    w = torch.zeros(8, dtype=torch.uint8)
    assert _lib.written(w, None, "x: workspace") is w and _lib.written(None, None, "x") is None
    for t, dt in ((w[1:], None), (base32[1:], torch.float32), (base64[1:], torch.int64)):
        with pytest.raises(ValueError, match='x: out must be 16-byte aligned'):
            _lib.written(t, dt, "x: out")
    with pytest.raises(ValueError, match='contiguous'):
        _lib.written(base32[::2], torch.float32, "x: out")
    # the last line of defence, and its opt-out
    assert _lib.ptr(base32).value == base32.data_ptr() and _lib.ptr(None) is None
    for call in (lambda: _lib.ptr(base32[1:]), lambda: _lib.ptr_array([base32, base32[1:]]), lambda: _lib.addr(base64[1:])):
        with pytest.raises(ValueError, match='not 16-byte aligned'):
            call()
    assert _lib.ptr(base32[1:], unaligned=True).value == base32.data_ptr() + 4
    assert list(_lib.ptr_array([base32[1:], None], unaligned=True)) == [base32.data_ptr() + 4, None]
    assert _lib.addr(base64[1:], unaligned=True) == base64.data_ptr() + 8 and _lib.addr(base64) == base64.data_ptr()
    # the spelling the wrappers use: one-argument calls of whatever `ptr` / `ptr_array` is at the moment, so that a guard that stands
    # in for them (also one written before the second argument existed) records the tensor; the opt-out ends with the call
    assert _lib.ptr_unaligned(base32[1:]).value == base32.data_ptr() + 4 and _lib.ptr_unaligned(None) is None
    assert list(_lib.ptr_array_unaligned([base32[1:], None])) == [base32.data_ptr() + 4, None]
    with pytest.raises(ValueError, match='not 16-byte aligned'):
        _lib.ptr(base32[1:])
    seen = []
    real = _lib.ptr
    try:
        _lib.ptr = lambda t: (seen.append(t), real(t))[1]          # a stand-in that takes one argument only
        off = base32[1:]
        assert _lib.ptr_unaligned(off).value == off.data_ptr() and seen == [off]
    finally:
        _lib.ptr = real
    logits, row, cls, out = _tensors()
    off_logits = torch.zeros(49)[1:].view(3, 4, 2, 2)
    with abiguard.guard(library=Stub()) as g:
        _gather(_lib.lib, lambda t: _lib.ptr_unaligned(t) if t is off_logits else _lib.ptr(t), off_logits, row, cls, out)
    assert g.launches() == 1 and not g.violations
    msg = _refused(lambda: _gather(_lib.lib, _lib.ptr_unaligned, logits, torch.zeros(6, dtype=torch.int32)[1:], cls, out), 'alignment', '(row)')
    assert '_lib.py' not in msg, "the site must be the caller's, not the binding's"


def test_the_offset_variant_builder():
    import test_abi_contract_gpu as contract
    make = contract.offset_variant
    for dt in (torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.int8, torch.bool, torch.int16, torch.bfloat16,
               torch.float16):
        t = (torch.arange(24) % 2 if dt == torch.bool else torch.arange(24)).to(dt).view(2, 3, 4)
        t.note = 'kept'
        v = make(t)
        assert v.dtype == dt and v.shape == t.shape and v.stride() == t.stride() and torch.equal(v, t) and v.note == 'kept'
        assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    x = torch.arange(2 * 3 * 2 * 2, dtype=torch.float32).view(2, 3, 2, 2).contiguous(memory_format=torch.channels_last)
    v = make(x)
    assert v.is_contiguous(memory_format=torch.channels_last) and not v.is_contiguous() and v.stride() == x.stride() and torch.equal(v, x)
    assert v.data_ptr() % 16 == 4
    one = torch.tensor([7], dtype=torch.int64)
    v = make(one)
    assert v.shape == (1,) and int(v[0]) == 7 and v.data_ptr() % 16 == 8
    assert make(torch.zeros(0)) is None and make(torch.zeros(3, 0, dtype=torch.int32)) is None
    rows = torch.arange(12.).view(3, 4)[:, :2]                       # a view with gaps keeps its pitch
    v = make(rows)
    assert v.stride() == rows.stride() and torch.equal(v, rows) and v.data_ptr() % 16 == 4
    assert dict(contract.VARIANTS)['offset'] is make and [n for n, _ in contract.VARIANTS] == ['strided', 'dtype', 'offset']


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
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in ('ptr', 'ptr_array', 'ptr_unaligned', 'ptr_array_unaligned') and n.args:
                a = n.args[0]
                if n.func.id.startswith('ptr_array') and isinstance(a, ast.Call) and isinstance(a.func, ast.Name) and a.func.id == 'list' and plain(a.args[0]):
                    continue
                if n.func.id.startswith('ptr_array') and isinstance(a, ast.BinOp):          # [None] * A
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
