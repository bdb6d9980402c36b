"""Test-side allocation guard: poison what the kernels get from torch.empty and fence it with guard bands.

Every HIP entry point of the package takes its outputs, split-K workspaces and weight packs from ``torch.empty``, and what a kernel
finds in memory it never writes is whatever the caching allocator had there. Inside ``poisoned(pattern)`` the ``torch`` name seen by
the allocating modules is a proxy that delegates everything but ``torch.empty``. MODULES is every module of the package with a function
that allocates, found by reading the package's files (scan_package): a new module enters by calling torch.empty. Each intercepted
allocation

  * is carved out of a larger uint8 buffer with a band of GUARD bytes before and after it (a multiple of 512: alignment is unchanged),
  * has the shape and strides of a ``device='meta'`` twin of the same call (channels_last, permuted views and zero-size results look
    exactly as torch's own),
  * is filled with the run's poison byte (PATTERNS, per dtype) while the bands hold GUARD_BYTE,
  * is recorded with its call site; on exit (after a synchronize) every band must still hold its byte, else AssertionError naming the
    call site and the first and last overwritten byte offsets relative to the allocation's start.

``banded_copy(x, pattern)`` places a test input inside bands of poison: an out-of-bounds read of an input that reaches a result then
changes the result between patterns A and B. Inside an active guard those bands are checked on exit too.

What the bands cannot see: stores through a buffer descriptor beyond its ``num_records`` (the hardware drops them, so nothing lands in
a band), and out-of-bounds reads whose value a select throws away (no value difference between patterns). Both are harmless to the
results, but they are invisible here; a wrong bounds rule of that kind needs a test of the rule itself.
"""
import ast
import contextlib
import importlib
import os
import sys

import torch

_REAL_EMPTY = torch.empty

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = 'upsnet_amd'
ALLOC_HELPERS = ('_ws', '_nhwc_out')                               # ops.py's two allocating helpers: their callers allocate
UNROUTED = ('empty_like', 'empty_strided', 'new_empty')            # uninitialised memory the proxy does not route


def scan_package():
    """What the package's Python files allocate, read from their syntax trees (nothing is imported):
    ({'upsnet_amd.x.y': {qualified name of every function / method}}, {'upsnet_amd.x.y': {those that allocate}},
    ['file:line: call' for every call of torch.empty_like, torch.empty_strided or <anything>.new_empty; numpy's host-side empty_like is
    not meant]).
    A function allocates if it calls torch.empty without pin_memory= (pinned host staging is no kernel's memory) or one of
    ALLOC_HELPERS, by its bare name or as an attribute (ops._nhwc_out); the helpers themselves are left out. A nested function counts for the function around it."""
    every, found, unrouted = {}, {}, []
    for dirpath, dirnames, filenames in os.walk(os.path.join(ROOT, PACKAGE)):
        dirnames.sort()
        for name in sorted(filenames):
            if not name.endswith('.py'):
                continue
            path = os.path.join(dirpath, name)
            rel = os.path.relpath(path, ROOT)
            parts = rel[:-3].split(os.sep)
            mod = '.'.join(parts[:-1] if parts[-1] == '__init__' else parts)
            with open(path) as f:
                tree = ast.parse(f.read(), rel)

            def allocates(fn):
                hit = False
                for n in ast.walk(fn):
                    if not isinstance(n, ast.Call):
                        continue
                    f = n.func
                    if isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id == 'torch' and f.attr == 'empty':
                        hit = hit or not any(k.arg == 'pin_memory' for k in n.keywords)
                    elif (f.id if isinstance(f, ast.Name) else f.attr if isinstance(f, ast.Attribute) else None) in ALLOC_HELPERS:
                        hit = True                # (_ws(...) inside ops.py, ops._nhwc_out(...) elsewhere)
                return hit

            def visit(node, prefix):
                for ch in ast.iter_child_nodes(node):
                    if isinstance(ch, ast.ClassDef):
                        visit(ch, prefix + ch.name + '.')
                    elif isinstance(ch, (ast.FunctionDef, ast.AsyncFunctionDef)):
                        every.setdefault(mod, set()).add(prefix + ch.name)
                        if ch.name not in ALLOC_HELPERS and allocates(ch):
                            found.setdefault(mod, set()).add(prefix + ch.name)
            visit(tree, '')
            calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in UNROUTED
                     and (n.func.attr == 'new_empty' or (isinstance(n.func.value, ast.Name) and n.func.value.id == 'torch'))]
            unrouted += ['%s:%d: %s' % (rel, n.lineno, ast.unparse(n.func)) for n in sorted(calls, key=lambda n: (n.lineno, n.col_offset))]
    return every, found, unrouted


# allocating modules that the guard does not import or patch: every allocating function of theirs is excluded from the sweep with a
# reason (tests/test_poisoned_memory_gpu.py: EXCLUDED; tests/test_memguard_cpu.py holds the two tables together)
UNGUARDED = ('upsnet_amd.upsnet_end2end_test',                  # the benchmark script: buffers of torch.distributed collectives
             'upsnet_amd.operators.modules.deform_conv')        # nn.Parameter storage, filled in the constructor

# every other module of the package with a function that allocates: a new one enters the guard (and the coverage check of
# tests/test_memguard_cpu.py) by calling torch.empty, _ws or _nhwc_out
MODULES = tuple(sorted(m for m in scan_package()[1] if m not in UNGUARDED))
GUARD = 4096
GUARD_BYTE = 0xA5

# pattern -> (byte for floating dtypes, byte for integer / bool dtypes). B keeps integers small: a stray index read from unwritten
# memory then lands inside a band (a value difference), not far away. 0x7F.. is a large finite float that fmaxf does not hide.
PATTERNS = {'A': (0xFF, 0xFF), 'B': (0x7F, 0x00)}

_ACTIVE = []          # guards in force (innermost last)


def poison_byte(dtype, pattern):
    fl, it = PATTERNS[pattern]
    return fl if (dtype.is_floating_point or dtype.is_complex) else it


def _call_site():
    f = sys._getframe(1)
    here = os.path.abspath(__file__)
    while f is not None and os.path.abspath(f.f_code.co_filename) == here:
        f = f.f_back
    if f is None:
        return '?'
    return '%s:%d (%s)' % (os.path.basename(f.f_code.co_filename), f.f_lineno, f.f_code.co_name)


def _extent_bytes(shape, stride, itemsize):
    if any(s == 0 for s in shape):
        return 0
    return (1 + sum((s - 1) * st for s, st in zip(shape, stride))) * itemsize


def _carve(shape, stride, dtype, device, fill, band, site, guard=None):
    """A tensor of (shape, stride, dtype) inside a uint8 buffer: [band x GUARD][fill x extent][band x GUARD]."""
    nbytes = _extent_bytes(shape, stride, torch.empty((), dtype=dtype, device='meta').element_size())
    buf = _REAL_EMPTY((GUARD + nbytes + GUARD,), dtype=torch.uint8, device=device)
    buf[:GUARD].fill_(band)
    buf[GUARD:GUARD + nbytes].fill_(fill)
    buf[GUARD + nbytes:].fill_(band)
    flat = buf[GUARD:GUARD + nbytes].view(dtype)
    t = flat.as_strided(tuple(shape), tuple(stride))
    if guard is not None:
        guard.records.append((buf, nbytes, band, site))
    return t


class Guard:
    def __init__(self, pattern, adopt=False):
        if pattern not in PATTERNS:
            raise ValueError("pattern must be one of %s" % sorted(PATTERNS))
        self.pattern = pattern
        self.adopt = adopt
        self.records = []      # (buffer, nbytes, band byte, call site)
        self.count = 0

    def empty(self, *size, **kw):
        if kw.get('out') is not None or kw.get('pin_memory') or kw.get('layout', torch.strided) != torch.strided:
            return _REAL_EMPTY(*size, **kw)        # host staging / out= / sparse: not a kernel's memory
        unknown = set(kw) - {'dtype', 'device', 'requires_grad', 'memory_format', 'layout', 'pin_memory', 'out'}
        if unknown:
            raise TypeError("memguard: unexpected torch.empty arguments %s" % sorted(unknown))
        dtype, device = kw.get('dtype'), kw.get('device')
        memory_format = kw.get('memory_format', torch.contiguous_format)
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        size = tuple(int(s) for s in size)
        dtype = dtype if dtype is not None else torch.get_default_dtype()
        device = torch.device(device) if device is not None else torch.device('cpu')
        twin = _REAL_EMPTY(size, dtype=dtype, device='meta', memory_format=memory_format)
        self.count += 1
        t = _carve(twin.shape, twin.stride(), dtype, device, poison_byte(dtype, self.pattern), GUARD_BYTE, _call_site(), self)
        return t.requires_grad_() if kw.get('requires_grad') else t

    def violations(self, first=0):
        """[(call site, first, last)] for every band (of the records from `first` on) that no longer holds its byte; offsets in bytes
        from the allocation's start."""
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            torch.cuda.synchronize()
        bad = []
        for buf, nbytes, band, site in self.records[first:]:
            head, tail = buf[:GUARD], buf[GUARD + nbytes:]
            if bool((head == band).all()) and bool((tail == band).all()):
                continue
            offs = torch.cat([torch.nonzero(head != band).flatten() - GUARD,
                              torch.nonzero(tail != band).flatten() + nbytes]).cpu()
            bad.append((site, int(offs.min()), int(offs.max())))
        return bad


class _Joined:
    """What a poisoned() inside an adopting guard yields: the outer guard's pattern and allocator, with the count, the records and the
    band check of the inner block alone."""

    def __init__(self, outer):
        self._outer, self._first, self._count0 = outer, len(outer.records), outer.count
        self.pattern = outer.pattern

    @property
    def count(self):
        return self._outer.count - self._count0

    @property
    def records(self):
        return self._outer.records[self._first:]

    def violations(self):
        return self._outer.violations(self._first)


class _TorchProxy:
    """The torch module with ``empty`` routed through a Guard."""

    def __init__(self, guard):
        self._guard = guard

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, **kw):
        return self._guard.empty(*args, **kw)


@contextlib.contextmanager
def poisoned(pattern, modules=MODULES, check=True, adopt=False):
    """Route torch.empty of ``modules`` through a Guard of ``pattern`` ('A' or 'B'); yields the Guard. The patch is undone on exit and
    on exception; on a normal exit the bands are checked (AssertionError on any overwritten band).

    adopt=True: a poisoned() entered while this guard is the innermost one joins it, whatever pattern it asks for: its modules are
    routed to this guard, and it yields a view of it with this guard's pattern and the inner block's own count, records and band
    check. A test body that poisons its own allocations (most feature tests do, under A and then B) then runs wholly under the outer
    pattern, and the two patterns are compared by whoever holds the outer guard, whose exit checks every band once more."""
    mods = [importlib.import_module(m) for m in modules]
    saved = [(m, m.__dict__.get('torch')) for m in mods]
    if _ACTIVE and _ACTIVE[-1].adopt:
        guard = _Joined(_ACTIVE[-1])
        proxy = _TorchProxy(_ACTIVE[-1])
        try:
            for m in mods:
                m.torch = proxy
            yield guard
        finally:
            for m, t in saved:
                m.torch = t
        if check:
            bad = guard.violations()
            assert not bad, "guard band overwritten: " + "; ".join("%s bytes [%d, %d]" % b for b in bad)
        return
    guard = Guard(pattern, adopt)
    proxy = _TorchProxy(guard)
    _ACTIVE.append(guard)
    try:
        for m in mods:
            m.torch = proxy
        yield guard
    finally:
        for m, t in saved:
            m.torch = t
        _ACTIVE.remove(guard)
    if check:
        bad = guard.violations()
        assert not bad, "guard band overwritten: " + "; ".join("%s bytes [%d, %d]" % b for b in bad)


def banded_copy(x, pattern):
    """A copy of ``x`` (same shape, strides where x is dense, dtype, device) inside bands of the pattern's poison byte; registered with
    the innermost active guard, whose exit then checks that those bands were not written."""
    twin = torch.empty_like(x, device='meta')
    byte = poison_byte(x.dtype, pattern)
    g = _ACTIVE[-1] if _ACTIVE else None
    t = _carve(twin.shape, twin.stride(), x.dtype, x.device, byte, byte, _call_site(), g)
    t.copy_(x)
    return t


def is_dense(t):
    """Non-overlapping and dense (a permutation of a contiguous layout): banded_copy keeps such a tensor's strides."""
    return t.numel() > 0 and all(st > 0 for s, st in zip(t.shape, t.stride()) if s > 1) and \
        _extent_bytes(t.shape, t.stride(), 1) == t.numel()


def bits(t):
    """The bytes of t in logical order (NaN == NaN, -0 != +0): for bitwise comparisons."""
    t = t.detach().contiguous().reshape(-1)
    if t.numel() == 0:
        return torch.empty((0,), dtype=torch.uint8, device=t.device)
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.view(torch.uint8)


def bit_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))
