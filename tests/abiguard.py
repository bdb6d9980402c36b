"""Test-side guard of the C-ABI boundary: what a wrapper hands to an ``extern "C"`` entry point of libupsnet_hip.so.

Every result of the package crosses one step that the kernel tests do not look at: a ``torch.Tensor`` becomes a raw address
(``_lib.ptr``, ``_lib.ptr_array``, ``_lib.addr``) and goes into a ctypes call whose parameter is a bare ``void *``. Three copies of each
signature exist (include/upsnet_hip.h, the definition in upsnet_amd/csrc, the ``argtypes`` row in upsnet_amd/_lib.py) and nothing
links them; a temporary's address outlives the temporary; an int32 tensor reads as int64 without complaint.

``header_abi()`` / ``definition_abi()`` / ``binding_abi()`` read the three copies (tests/test_abiguard_cpu.py compares them).

Inside ``guard()``
  * ``ptr`` / ``ptr_array`` / ``addr`` of ``upsnet_amd._lib`` -- and of every module of the package that imported them by name
    (``holders()`` finds those by reading the package's files) -- return what the originals return and note, per address, a weak
    reference to the tensor with its dtype, shape, strides, device and the call site;
  * ``_lib.lib()`` is a proxy: before the real entry point is called, every argument that the header declares a pointer is checked
    (RULES below), and a broken rule raises AbiViolation naming symbol, parameter, call site and rule. Nothing is launched then.
    ``Guard.calls`` counts, per symbol, the calls that did go through, ``Guard.violations`` keeps every message (a test body that
    expects an exception of its own must not be able to swallow one).

Rules for a non-NULL pointer argument (``stream`` and ctypes host arrays -- int_array, float_array -- are exempt):
  origin    its address came out of ptr / ptr_array / addr;
  liveness  the tensor behind it is alive (a dead weak reference: "freed before launch");
  type      float -> float32, double -> float64, int / unsigned -> int32, int64_t / long -> int64, (unsigned) char -> uint8 / int8 /
            bool, unsigned short and the 16-bit typedefs -> bfloat16 / float16 / int16 / uint16, void -> anything;
  density   the tensor is contiguous in some memory format, or (symbol, parameter) is in STRIDED with the stride parameter named;
  device    a CUDA tensor lives on torch.cuda.current_device() (``stream()`` is that device's stream);
  alignment its address is a multiple of 16, or (symbol, parameter) is in UNALIGNED: the parameters whose kernels were read and found
            to access them at element width only. Host parameters (``*_host``, HOST) are outside this rule.

What the guard cannot know is how many bytes an entry point reads (the guard bands of tests/memguard.py cover that).
"""
import ast
import collections
import contextlib
import ctypes
import functools
import importlib
import os
import re
import sys
import weakref

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = 'upsnet_amd'
HEADER = os.path.join('include', 'upsnet_hip.h')
POINTER_MAKERS = ('ptr', 'ptr_array', 'addr')       # the functions of _lib that turn a tensor into an address
PATCHED = POINTER_MAKERS + ('lib',)                 # what guard() replaces wherever the package holds it


class AbiViolation(Exception):
    """A pointer argument of an entry point breaks a rule. Deliberately none of ValueError / TypeError / RuntimeError: those are a
    wrapper's own refusals."""


# ------------------------------------------------------------------------------------------------ the three copies of a signature
_QUALIFIERS = {'const', '__restrict__', '__restrict', 'restrict', 'volatile'}
_BASE = {('unsigned', 'char'): 'unsigned char', ('signed', 'char'): 'char', ('unsigned', 'short'): 'unsigned short',
         ('unsigned', 'int'): 'unsigned', ('long', 'long'): 'long', ('unsigned', 'long'): 'size_t', ('long', 'int'): 'long'}


def _strip_comments(text):
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    return re.sub(r'^[ \t]*#[^\n]*(\\\n[^\n]*)*', ' ', text, flags=re.M)


def _norm(base):
    """The fixed-width typedefs of <stdint.h> as the plain types they are on the one platform the library is built for (LP64)."""
    return {'int64_t': 'long', 'uint16_t': 'unsigned short', 'uint8_t': 'unsigned char', 'int8_t': 'char', 'int32_t': 'int',
            'int16_t': 'short', 'uint32_t': 'unsigned', 'uint64_t': 'size_t'}.get(base, base)


def _ctype(tokens, stars):
    words = [t for t in tokens if t not in _QUALIFIERS]
    base = _BASE.get(tuple(words), ' '.join(words))
    return _norm(base) + '*' * stars


def _parse_param(text):
    """'const float *const feat[4]' -> ('feat', 'float**'); 'int n' -> ('n', 'int'); 'void *' -> ('', 'void*')."""
    text = text.strip()
    stars = text.count('*') + len(re.findall(r'\[[^\]]*\]', text))
    text = re.sub(r'\[[^\]]*\]', ' ', text).replace('*', ' ')
    words = [w for w in text.split() if w not in _QUALIFIERS]
    name = ''
    if len(words) >= 2 and words[-1] not in ('char', 'short', 'int', 'long', 'float', 'double', 'void'):
        name = words.pop()
    return name, _ctype(words, stars)


def _parse_signatures(text, terminator):
    """{symbol: [(return type, [(name, type)])]} of every `type upsnet_x(params)` followed by `terminator` (';' a declaration, '{' a
    definition) in comment-free C text."""
    out = collections.OrderedDict()
    pat = re.compile(r'((?:\b[A-Za-z_]\w*\b[\s\*]+)+?)(upsnet_\w+)\s*\(([^()]*)\)\s*' + re.escape(terminator))
    for m in pat.finditer(text):
        ret_words = m.group(1).replace('*', ' * ').split()
        ret_words = [w for w in ret_words if w not in ('extern', 'static', 'inline')]
        if not ret_words or ret_words[0] in ('return', 'else', 'case', 'goto'):
            continue
        ret = _ctype([w for w in ret_words if w != '*'], ret_words.count('*'))
        params = m.group(3).strip()
        plist = [] if params in ('', 'void') else [_parse_param(p) for p in params.split(',')]
        out.setdefault(m.group(2), []).append((ret, plist))
    return out


@functools.lru_cache(maxsize=None)
def _header_abi(path):
    """{symbol: (return type, [(parameter name, C type)])} of include/upsnet_hip.h, comments stripped. A type is a scalar ('int',
    'float', 'double', 'long', 'size_t', ...) or a pointer spelled with its element type ('float*', 'void*', 'float**'); `int64_t` reads
    'long', const and restrict are dropped, an array parameter (`const float w[4]`) is a pointer."""
    with open(path) as f:
        text = _strip_comments(f.read())
    text = text.replace('extern "C" {', ' ')
    found = _parse_signatures(text, ';')
    dup = sorted(s for s, v in found.items() if len(v) > 1)
    if dup:
        raise ValueError("declared more than once in the header: %s" % dup)
    return collections.OrderedDict((s, v[0]) for s, v in found.items())


def header_abi(path=None):
    """(read once per file and process: a guard is entered for every replay of the form sweep)"""
    return collections.OrderedDict(_header_abi(path or os.path.join(ROOT, HEADER)))


def definition_abi(root=None):
    """{symbol: [(file, return type, [(name, type)])]} of every extern "C" definition of an upsnet_* symbol in csrc/*.hip, *.cpp."""
    d = os.path.join(root or ROOT, PACKAGE, 'csrc')
    out = {}
    for name in sorted(os.listdir(d)):
        if not name.endswith(('.hip', '.cpp')):
            continue
        with open(os.path.join(d, name)) as f:
            text = _strip_comments(f.read())
        for m in re.finditer(r'extern\s+"C"\s+(?!\{)', text):
            head = text[m.end():]
            stop = re.search(r'[;{]', head)
            if stop is None or head[stop.start()] != '{':
                continue                                            # a declaration
            for sym, sigs in _parse_signatures(head[:stop.start() + 1], '{').items():
                out.setdefault(sym, []).append((name,) + sigs[0])
    return out


_CTYPES_NAME = {ctypes.c_int: 'c_int', ctypes.c_float: 'c_float', ctypes.c_double: 'c_double', ctypes.c_long: 'c_long',
                ctypes.c_size_t: 'c_size_t', ctypes.c_void_p: 'c_void_p', ctypes.c_char_p: 'c_char_p', None: 'None'}
# (c_size_t is c_ulong and c_long is c_long here; where a platform aliases two of them, the later name wins for both, consistently)


def binding_name(c_type, is_result=False):
    """The ctypes spelling that a header type must have in _lib._SIGNATURES."""
    if c_type.endswith('*'):
        return 'c_char_p' if (is_result and c_type == 'char*') else 'c_void_p'
    return {'int': 'c_int', 'unsigned': 'c_int', 'float': 'c_float', 'double': 'c_double', 'long': 'c_long', 'size_t': 'c_size_t',
            'void': 'None'}.get(c_type, '?' + c_type)


def binding_abi(signatures=None):
    """{symbol: (result name, [argument names])} of upsnet_amd._lib._SIGNATURES, in ctypes spelling."""
    if signatures is None:
        from upsnet_amd import _lib
        signatures = _lib._SIGNATURES
    return {s: (_CTYPES_NAME.get(res, repr(res)), [_CTYPES_NAME.get(a, repr(a)) for a in args]) for s, (res, args) in signatures.items()}


def signature_mismatches(header=None, definitions=None, binding=None):
    """Every disagreement of the three copies, one line each: 'symbol: parameter k (name): header says X, <copy> says Y'."""
    header = header_abi() if header is None else header
    definitions = definition_abi() if definitions is None else definitions
    binding = binding_abi() if binding is None else binding
    bad = []
    for sym in sorted(set(header) | set(definitions) | set(binding)):
        if sym not in header:
            bad.append("%s: not declared in the header (%s)" % (sym, 'defined in ' + definitions[sym][0][0] if sym in definitions else 'bound in _lib'))
            continue
        h_ret, h_par = header[sym]
        defs = definitions.get(sym, [])
        if len(defs) != 1:
            bad.append("%s: %d definitions (%s), exactly one wanted" % (sym, len(defs), ', '.join(d[0] for d in defs) or 'none'))
        for fname, d_ret, d_par in defs:
            if d_ret != h_ret:
                bad.append("%s: result: header says %s, %s says %s" % (sym, h_ret, fname, d_ret))
            if len(d_par) != len(h_par):
                bad.append("%s: header has %d parameters, %s has %d" % (sym, len(h_par), fname, len(d_par)))
            for k, ((hn, ht), (dn, dt)) in enumerate(zip(h_par, d_par)):
                if ht != dt:
                    bad.append("%s: parameter %d (%s): header says %s, %s says %s (%s)" % (sym, k, hn, ht, fname, dt, dn))
                    break                                           # (every later one is shifted: one line per symbol and copy)
        if sym not in binding:
            bad.append("%s: no row in _lib._SIGNATURES" % sym)
            continue
        b_ret, b_par = binding[sym]
        if binding_name(h_ret, True) != b_ret:
            bad.append("%s: result: header says %s (%s), _SIGNATURES says %s" % (sym, h_ret, binding_name(h_ret, True), b_ret))
        if len(b_par) != len(h_par):
            bad.append("%s: header has %d parameters, _SIGNATURES has %d" % (sym, len(h_par), len(b_par)))
        for k, ((hn, ht), bt) in enumerate(zip(h_par, b_par)):
            if binding_name(ht) != bt:
                bad.append("%s: parameter %d (%s): header says %s (%s), _SIGNATURES says %s" % (sym, k, hn, ht, binding_name(ht), bt))
                break
    return bad


# ------------------------------------------------------------------------------------------------ the package's files
def _package_files():
    for dirpath, dirnames, filenames in os.walk(os.path.join(ROOT, PACKAGE)):
        dirnames.sort()
        for name in sorted(filenames):
            if name.endswith('.py'):
                path = os.path.join(dirpath, name)
                rel = os.path.relpath(path, ROOT)
                parts = rel[:-3].split(os.sep)
                yield path, rel, '.'.join(parts[:-1] if parts[-1] == '__init__' else parts)


def _qualified_functions(tree):
    """[(qualified name, FunctionDef)] of the functions and methods of a module; a nested function counts for the one around it."""
    out = []

    def visit(node, prefix):
        for ch in ast.iter_child_nodes(node):
            if isinstance(ch, ast.ClassDef):
                visit(ch, prefix + ch.name + '.')
            elif isinstance(ch, (ast.FunctionDef, ast.AsyncFunctionDef)):
                out.append((prefix + ch.name, ch))
    visit(tree, '')
    return out


@functools.lru_cache(maxsize=None)
def scan_package():
    """Read from the syntax trees of the package's files (nothing is imported):
    holders    {'upsnet_amd.x': {names among POINTER_MAKERS that the module imports from _lib by name}},
    callers    {'upsnet_amd.x': {qualified function: {upsnet_* symbols its body calls}}},
    every      {'upsnet_amd.x': {qualified name of every function / method}},
    data_ptrs  [(file, line, qualified function or '<module>', source of the statement)] for every .data_ptr() outside _lib.py."""
    holders, callers, every, data_ptrs = {}, {}, {}, []
    for path, rel, mod in _package_files():
        with open(path) as f:
            src = f.read()
        tree = ast.parse(src, rel)
        for n in ast.walk(tree):
            if isinstance(n, ast.ImportFrom) and n.module is not None and n.module.split('.')[-1] == '_lib':
                names = {a.asname or a.name for a in n.names if a.name in PATCHED}
                if names:
                    holders.setdefault(mod, set()).update(names)
        funcs = _qualified_functions(tree)
        for q, fn in funcs:
            every.setdefault(mod, set()).add(q)
            syms = {n.func.attr for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)
                    and n.func.attr.startswith('upsnet_')}
            if syms:
                callers.setdefault(mod, {})[q] = syms
        if os.path.basename(path) == '_lib.py':
            continue
        lines = src.splitlines()
        spans = [(fn.lineno, fn.end_lineno, q) for q, fn in funcs]
        for n in ast.walk(tree):
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == 'data_ptr':
                inside = [q for lo, hi, q in spans if lo <= n.lineno <= hi]
                data_ptrs.append((rel, n.lineno, inside[-1] if inside else '<module>', lines[n.lineno - 1].strip()))
    return holders, callers, every, sorted(data_ptrs)


def holders():
    """The modules whose namespace holds ptr / ptr_array / addr: _lib itself and everyone who imported one of them by name."""
    found = dict(scan_package()[0])
    found[PACKAGE + '._lib'] = set(PATCHED)
    return found


def pointer_callers(header=None):
    """{'module.qualname' (module's last name component)} of every function of the package whose body calls an upsnet_* symbol with at
    least one pointer parameter besides `stream`, and the same for every function at all."""
    header = header_abi() if header is None else header
    with_ptr = {s for s, (_, params) in header.items() if any(t.endswith('*') and n != 'stream' for n, t in params)}
    _, callers, every, _ = scan_package()
    found = {m.rsplit('.', 1)[-1] + '.' + q for m, fs in callers.items() for q, syms in fs.items() if syms & with_ptr}
    flat = {m.rsplit('.', 1)[-1] + '.' + q for m, qs in every.items() for q in qs}
    return found, flat


# ------------------------------------------------------------------------------------------------ the rules
ELEMENT_DTYPES = {
    'float': (torch.float32,), 'double': (torch.float64,), 'int': (torch.int32,), 'unsigned': (torch.int32,),
    'long': (torch.int64,), 'unsigned char': (torch.uint8, torch.int8, torch.bool), 'char': (torch.uint8, torch.int8, torch.bool),
    'unsigned short': (torch.bfloat16, torch.float16, torch.int16) + ((torch.uint16,) if hasattr(torch, 'uint16') else ()),
    'short': (torch.int16,), 'size_t': (torch.int64,), 'void': None,
}

# (symbol, parameter) pairs that may be given a view that is contiguous in no memory format, each with the stride parameter the entry
# point takes for it
STRIDED = {
    ('upsnet_mask_logit_gather', 'mask_logit'): "rows, classes and elements at stride_n / stride_c / stride_e elements",
    ('upsnet_pyramid_proposals_strided', 'cls_prob'): "each level's scores at cls_chan_stride[l] / cls_pix_stride[l] elements",
    ('upsnet_pyramid_proposals_strided', 'bbox_pred'): "each level's deltas at box_chan_stride[l] / box_pix_stride[l] elements",
    ('upsnet_pyramid_proposals_strided_ordered', 'cls_prob'): "each level's scores at cls_chan_stride[l] / cls_pix_stride[l] elements",
    ('upsnet_pyramid_proposals_strided_ordered', 'bbox_pred'): "each level's deltas at box_chan_stride[l] / box_pix_stride[l] elements",
    ('upsnet_pyramid_proposals_joint_strided', 'cls_prob'): "each level's scores at cls_chan_stride[l] / cls_pix_stride[l] elements",
    ('upsnet_pyramid_proposals_joint_strided', 'bbox_pred'): "each level's deltas at box_chan_stride[l] / box_pix_stride[l] elements",
    ('upsnet_restore_label_maps', 'sseg'): "rows of the source map at src_stride elements (a crop of a padded map)",
    ('upsnet_restore_label_maps', 'pano'): "rows of the source map at src_stride elements (a crop of a padded map)",
    ('upsnet_restore_plane_u8', 'src'): "rows of the source plane at src_stride bytes (a crop of a padded plane)",
}

# (symbol, parameter) pairs that may be given an address that is only element-aligned (a view that starts inside an allocation), each
# with the reading that allows it: in every kernel the entry point launches, every access through the pointer is one element wide, and
# no pointer derived from it is reinterpreted wider or used for an atomic. Everything else -- every output, workspace, accumulator and
# counter in particular -- is held to ALIGN bytes without a reading. None of the HOST / *_host parameters is read by a kernel directly:
# each feeds a copy or host-side launch arithmetic.
ALIGN = 16
UNALIGNED = {
    ('upsnet_mask_logit_gather', 'mask_logit'): "detect.hip mask_logit_gather_kernel: one float load sp[e * s_e] per output element, nothing wider",
    ('upsnet_pyramid_proposals_strided', 'cls_prob'): "forwards to _strided_ordered: proposal.hip reads s[a * cs + pix * ps], one float per key",
    ('upsnet_pyramid_proposals_strided', 'bbox_pred'): "forwards to _strided_ordered: proposal.hip reads d[0], d[bcs], d[2 bcs], d[3 bcs] as single floats",
    ('upsnet_pyramid_proposals_strided_ordered', 'cls_prob'): "proposal.hip key kernels read s[a * cs + pix * ps], one float per key, nothing wider",
    ('upsnet_pyramid_proposals_strided_ordered', 'bbox_pred'): "proposal.hip decode reads d[0], d[bcs], d[2 bcs], d[3 bcs] as single floats at a run-time stride",
    ('upsnet_pyramid_proposals_joint_strided', 'cls_prob'): "proposal.hip joint key kernel reads s[a * cs + pix * ps], one float per key, nothing wider",
    ('upsnet_pyramid_proposals_joint_strided', 'bbox_pred'): "proposal.hip decode reads d[0], d[bcs], d[2 bcs], d[3 bcs] as single floats at a run-time stride",
    ('upsnet_restore_label_maps', 'sseg'): "restore.hip rs_gather_chunk: one int64 load row[sx] per output byte; the 16-byte store is on the output",
    ('upsnet_restore_label_maps', 'pano'): "restore.hip rs_gather_chunk: one int64 load row[sx] per output byte; the 16-byte store is on the output",
    ('upsnet_restore_plane_u8', 'src'): "restore.hip rs_gather_chunk: one byte load row[sx] per output byte; the 16-byte store is on the output",
}

# pointer parameters that take HOST memory although their name does not end in _host (the header's convention for host pointers):
# numpy buffers that the entry point reads before it returns. The origin rule does not apply to them.
HOST = {
    ('upsnet_vis_font', 'cells'): "host buffer the glyph cells are copied into (dataset/vis.py reads them back as numpy)",
    ('upsnet_poly_raster', 'poly_off'): "host copy of the polygon offsets, read while the launch is sized (the device copy is poly_off_dev)",
    ('upsnet_poly_raster', 'obj_off'): "host copy of the object offsets, read while the launch is sized (the device copy is obj_off_dev)",
}

Record = collections.namedtuple('Record', 'ref base dtype shape stride device site address')


def _site():
    f = sys._getframe(1)
    here = os.path.abspath(__file__)
    # (the binding's own frames are skipped too: ptr_unaligned / ptr_array_unaligned call ptr on the wrapper's behalf)
    while f is not None and (os.path.abspath(f.f_code.co_filename) == here or os.path.basename(f.f_code.co_filename) == '_lib.py'):
        f = f.f_back
    if f is None:
        return '?'
    return '%s:%d (%s)' % (os.path.basename(f.f_code.co_filename), f.f_lineno, f.f_code.co_name)


def _record(t, site):
    base = t._base                                   # (a view keeps its base's memory alive: x[b:] may die, x must not)
    return Record(weakref.ref(t), None if base is None else weakref.ref(base), t.dtype, tuple(t.shape), tuple(t.stride()), t.device, site,
                  t.data_ptr())


def _some_memory_format(shape, stride):
    t = torch.empty_strided(shape, stride, device='meta')
    if t.numel() <= 1 or t.is_contiguous():
        return True
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return True
    return t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d)


def _current_device():
    return torch.cuda.current_device()


class Guard:
    def __init__(self, header, strided, unaligned=None):
        self.header = header
        self.strided = strided
        self.unaligned = UNALIGNED if unaligned is None else unaligned
        self.registry = {}                          # address -> Record (the latest ptr() of that address)
        self.calls = collections.Counter()          # symbol -> calls that reached the library
        self.violations = []
        self.on_call = None                         # optional hook (symbol, args) -> None, called after the checks, before the library

    # ---- the replacements of _lib.ptr / ptr_array / addr
    def make_ptr(self, real):
        def ptr(t, unaligned=False):
            p = real(t, unaligned) if unaligned else real(t)       # (a tree from before the rule has no such argument, and no caller of it)
            if t is not None:
                rec = _record(t, _site())
                self.registry[rec.address] = rec
                p._abiguard = rec
            return p
        return ptr

    def make_ptr_array(self, real):
        def ptr_array(tensors, unaligned=False):
            tensors = list(tensors)
            arr = real(tensors, unaligned) if unaligned else real(tensors)
            site = _site()
            recs = [None if t is None else _record(t, site) for t in tensors]
            for r in recs:
                if r is not None:
                    self.registry[r.address] = r
            arr._abiguard = recs
            return arr
        return ptr_array

    def make_addr(self, real):
        def addr(t, unaligned=False):
            a = real(t, unaligned) if unaligned else real(t)
            rec = _record(t, _site())
            self.registry[rec.address] = rec
            return a
        return addr

    # ---- the checks
    def _fail(self, sym, pname, site, rule, detail):
        msg = "%s(%s) <- %s: %s: %s" % (sym, pname, site, rule, detail)
        self.violations.append(msg)
        raise AbiViolation(msg)

    def _check_record(self, sym, pname, elem, rec, key=None):
        if rec.ref() is None and (rec.base is None or rec.base() is None):
            self._fail(sym, pname, rec.site, 'liveness', "the %s tensor %s behind 0x%x was freed before launch"
                       % (str(rec.dtype).replace('torch.', ''), rec.shape, rec.address))
        want = ELEMENT_DTYPES.get(elem, ())
        if want is not None and rec.dtype not in want:
            self._fail(sym, pname, rec.site, 'element type', "the header says %s *, the tensor is %s (wanted %s)"
                       % (elem, rec.dtype, ' / '.join(str(w) for w in want) or 'a type the guard knows'))
        if not _some_memory_format(rec.shape, rec.stride) and (sym, key or pname) not in self.strided:
            self._fail(sym, pname, rec.site, 'density', "shape %s with strides %s is contiguous in no memory format, and the pair is "
                       "not in abiguard.STRIDED" % (rec.shape, rec.stride))
        if rec.device.type == 'cuda' and rec.device.index != _current_device():
            self._fail(sym, pname, rec.site, 'device', "the tensor is on %s, the current device (whose stream the call gets) is cuda:%d"
                       % (rec.device, _current_device()))
        if rec.address % ALIGN and (sym, key or pname) not in self.unaligned:
            self._fail(sym, pname, rec.site, 'alignment', "0x%x is %d bytes past a multiple of %d (%s %s, a view that starts inside an "
                       "allocation?), and the pair is not in abiguard.UNALIGNED" % (rec.address, rec.address % ALIGN, ALIGN,
                                                                                   str(rec.dtype).replace('torch.', ''), rec.shape))

    def check_call(self, sym, args):
        ret, params = self.header[sym]
        if len(args) != len(params):
            raise TypeError("%s takes %d arguments (include/upsnet_hip.h), %d given" % (sym, len(params), len(args)))
        for (pname, ctype), a in zip(params, args):
            if not ctype.endswith('*') or pname == 'stream' or a is None:
                continue
            elem, depth = ctype.rstrip('*'), len(ctype) - len(ctype.rstrip('*'))
            if isinstance(a, ctypes.Array):
                recs = getattr(a, '_abiguard', None)
                if recs is not None:
                    for i, r in enumerate(recs):
                        if r is not None:
                            self._check_record(sym, '%s[%d]' % (pname, i), elem, r, pname)
                elif depth >= 2 and a._type_ is ctypes.c_void_p:
                    for i, v in enumerate(a):
                        if v:
                            self._by_address(sym, '%s[%d]' % (pname, i), elem, int(v), pname)
                continue                                            # (int_array, float_array and their like: host arrays of scalars)
            if pname.endswith('_host') or (sym, pname) in HOST:
                continue                                            # (host memory by the header's convention / by the HOST table)
            rec = getattr(a, '_abiguard', None)
            if rec is not None:
                self._check_record(sym, pname, elem, rec)
                continue
            value = a.value if isinstance(a, ctypes.c_void_p) else a
            if isinstance(value, int):
                if value:
                    self._by_address(sym, pname, elem, value)
                continue
            if isinstance(a, (bytes, ctypes.c_char_p)) or type(a).__name__ in ('CArgObject',):
                continue                                            # (a host string / byref of a host scalar)
            self._fail(sym, pname, '?', 'origin', "a %s is no address that ptr / ptr_array / addr made" % type(a).__name__)

    def _by_address(self, sym, pname, elem, address, key=None):
        rec = self.registry.get(address)
        if rec is None:
            self._fail(sym, pname, '?', 'origin', "0x%x was not made by ptr / ptr_array / addr" % address)
        self._check_record(sym, pname, elem, rec, key)

    def launches(self):
        """The calls that went through to an entry point with a pointer parameter (size queries and tuning knobs are no launches)."""
        return sum(n for s, n in self.calls.items() if any(t.endswith('*') for _, t in self.header[s][1]))


class _LibProxy:
    def __init__(self, real, guard):
        self._real, self._guard = real, guard

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith('upsnet_') or name not in self._guard.header:
            return fn
        g = self._guard

        def entry(*args):
            g.check_call(name, args)
            if g.on_call is not None:
                g.on_call(name, args)
            g.calls[name] += 1
            return fn(*args)
        entry.__name__ = name
        return entry


@contextlib.contextmanager
def guard(library=None, strided=None, unaligned=None):
    """Patch ptr / ptr_array / addr and lib in upsnet_amd._lib and in every module that imported them by name; yields the Guard.
    `library`: an object standing in for the loaded library (CPU tests); default: the real one, loaded on first use."""
    lib_mod = importlib.import_module(PACKAGE + '._lib')
    g = Guard(header_abi(), STRIDED if strided is None else strided, unaligned)
    found = holders()
    mods = {m: importlib.import_module(m) for m in found}
    makers = {'ptr': g.make_ptr, 'ptr_array': g.make_ptr_array, 'addr': g.make_addr}
    repl = {n: makers[n](getattr(lib_mod, n)) for n in POINTER_MAKERS if hasattr(lib_mod, n)}
    real_lib = lib_mod.lib
    proxy = {}

    def lib():
        if 'p' not in proxy:
            proxy['p'] = _LibProxy(library if library is not None else real_lib(), g)
        return proxy['p']

    saved = []
    try:
        for name, m in mods.items():
            for n in sorted(found[name]):
                if n == 'lib' and name != lib_mod.__name__:
                    if m.__dict__.get('lib') is real_lib:
                        saved.append((m, 'lib', real_lib))
                        m.lib = lib
                elif n in repl and n in m.__dict__:
                    saved.append((m, n, m.__dict__[n]))
                    setattr(m, n, repl[n])
        saved.append((lib_mod, 'lib', real_lib))
        lib_mod.lib = lib
        yield g
    finally:
        for m, n, v in reversed(saved):
            setattr(m, n, v)
