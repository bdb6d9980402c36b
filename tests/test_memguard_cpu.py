"""CPU: tests/memguard.py itself -- poison fill, torch's own shapes and strides, band violations with their call site, the patch undone
on every exit -- and the coverage check: every allocating entry point of the package has a case in tests/test_poisoned_memory_gpu.py or
a reasoned exclusion."""
import ast
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import memguard  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16, torch.float64, torch.int32, torch.int64, torch.uint8]


@pytest.fixture
def fake_module(monkeypatch):
    """A stand-in allocating module: memguard patches its `torch` name like the package's."""
    import types
    m = types.ModuleType('memguard_fake_mod')
    m.torch = torch
    exec("def alloc(*a, **k):\n    return torch.empty(*a, **k)\n", m.__dict__)
    monkeypatch.setitem(sys.modules, 'memguard_fake_mod', m)
    return m


@pytest.mark.parametrize("pattern", ['A', 'B'])
@pytest.mark.parametrize("dtype", DTYPES)
def test_allocations_hold_the_pattern(fake_module, pattern, dtype):
    with memguard.poisoned(pattern, modules=('memguard_fake_mod',)) as g:
        t = fake_module.alloc((3, 5, 7), dtype=dtype)
    assert g.count == 1
    want = memguard.poison_byte(dtype, pattern)
    assert want == (0xFF if pattern == 'A' else (0x7F if dtype.is_floating_point else 0x00))
    b = memguard.bits(t)
    assert b.numel() == t.numel() * t.element_size() and bool((b == want).all())
    if dtype == torch.float32:
        assert (torch.isnan(t).all() if pattern == 'A' else (torch.isfinite(t) & (t > 3e38)).all())


@pytest.mark.parametrize("args,kw,post", [
    (((2, 3, 4, 5),), {}, None),
    ((2, 3, 4, 5), {}, None),
    (((2, 3, 4, 5),), {'memory_format': torch.channels_last}, None),
    (((2, 5, 4, 3),), {}, lambda t: t.permute(0, 3, 1, 2)),
    (((0, 3),), {}, None),
    (((4, 0, 2, 2),), {'memory_format': torch.channels_last}, None),
    (((1, 0, 2, 3),), {}, lambda t: t.permute(0, 3, 1, 2)),
    ((7,), {'dtype': torch.int64}, None),
    (((),), {}, None),
])
def test_shapes_and_strides_match_torch(fake_module, args, kw, post):
    ref = torch.empty(*args, **kw)
    with memguard.poisoned('A', modules=('memguard_fake_mod',)):
        t = fake_module.alloc(*args, **kw)
    if post is not None:
        ref, t = post(ref), post(t)
    assert t.shape == ref.shape and t.stride() == ref.stride() and t.dtype == ref.dtype
    assert t.is_contiguous() == ref.is_contiguous()
    assert t.is_contiguous(memory_format=torch.channels_last) == ref.is_contiguous(memory_format=torch.channels_last)
    assert t.storage_offset() * t.element_size() == memguard.GUARD and memguard.GUARD % 512 == 0


def _raw(t):
    """The whole uint8 buffer an allocation was carved from."""
    return torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage())


@pytest.mark.parametrize("where,first", [('before', -1), ('after', 0), ('far', 100)])
def test_band_write_is_reported_with_its_call_site(fake_module, where, first):
    with pytest.raises(AssertionError) as e:
        with memguard.poisoned('B', modules=('memguard_fake_mod',)):
            t = fake_module.alloc((5, 3), dtype=torch.float32)
            raw = _raw(t)
            if where == 'before':
                raw[memguard.GUARD - 1] = 0
            elif where == 'after':
                raw[memguard.GUARD + 60] = 0
            else:
                raw[memguard.GUARD + 60 + 100] = 1
                raw[memguard.GUARD + 60 + 300] = 1
    msg = str(e.value)
    assert "alloc" in msg, msg
    lo = first if where == 'before' else 60 + first
    hi = {'before': -1, 'after': 60, 'far': 360}[where]
    assert "bytes [%d, %d]" % (lo, hi) in msg, msg


def test_writes_inside_the_allocation_are_fine(fake_module):
    with memguard.poisoned('A', modules=('memguard_fake_mod',)):
        t = fake_module.alloc((4, 4), dtype=torch.int32)
        t.fill_(3)
        x = memguard.banded_copy(torch.arange(6.0).view(2, 3), 'A')
    assert bool((t == 3).all()) and torch.equal(x, torch.arange(6.0).view(2, 3))


def test_banded_copy_sits_in_poison_and_its_bands_are_checked():
    x = torch.randn(2, 3, 4, 5).contiguous(memory_format=torch.channels_last)
    for pattern in 'AB':
        c = memguard.banded_copy(x, pattern)
        assert torch.equal(c, x) and c.stride() == x.stride()
        raw = _raw(c)
        byte = memguard.poison_byte(x.dtype, pattern)
        n = x.numel() * 4
        assert bool((raw[:memguard.GUARD] == byte).all()) and bool((raw[memguard.GUARD + n:] == byte).all())
    with pytest.raises(AssertionError, match="test_banded_copy"):
        with memguard.poisoned('A', modules=()):
            c = memguard.banded_copy(x, 'A')
            _raw(c)[memguard.GUARD + x.numel() * 4] = 0


def test_patch_is_undone_on_exit_and_on_exception(fake_module):
    mods = [__import__(m, fromlist=['_']) for m in memguard.MODULES]
    with memguard.poisoned('A') as g:
        assert all(m.torch is not torch for m in mods)
        assert mods[0].torch.float32 is torch.float32 and mods[0].torch.Tensor is torch.Tensor
    assert all(m.torch is torch for m in mods) and g.count == 0
    with pytest.raises(ZeroDivisionError):
        with memguard.poisoned('B', modules=memguard.MODULES + ('memguard_fake_mod',)):
            fake_module.alloc(3)
            1 / 0
    assert all(m.torch is torch for m in mods) and fake_module.torch is torch
    assert not memguard._ACTIVE
    assert torch.empty is memguard._REAL_EMPTY
    # host pinned / out= allocations pass through untouched
    with memguard.poisoned('A', modules=('memguard_fake_mod',)) as g:
        o = torch.zeros(3)
        fake_module.alloc(3, out=o)
    assert g.count == 0


# ---------------------------------------------------------------- coverage of the allocating entry points
ALLOC_FILES = ('upsnet_amd/ops.py', 'upsnet_amd/dataset/coco_eval.py', 'upsnet_amd/dataset/rle.py')
ALLOC_CALLS = {'empty', '_ws', '_nhwc_out'}


def allocating_functions():
    """({'module.qualname'} of every function / method in ALLOC_FILES that calls torch.empty, _ws or _nhwc_out (the two helpers
    excluded), {'module.qualname'} of every function / method there)."""
    found, every = set(), set()
    for rel in ALLOC_FILES:
        mod = os.path.splitext(os.path.basename(rel))[0]
        with open(os.path.join(ROOT, rel)) as f:
            tree = ast.parse(f.read())

        def visit(node, prefix):
            for ch in ast.iter_child_nodes(node):
                if isinstance(ch, ast.ClassDef):
                    visit(ch, prefix + ch.name + '.')
                elif isinstance(ch, ast.FunctionDef):
                    every.add(mod + '.' + prefix + ch.name)
                    for n in ast.walk(ch):
                        if isinstance(n, ast.Call):
                            fn = n.func
                            name = fn.attr if (isinstance(fn, ast.Attribute) and isinstance(fn.value, ast.Name) and fn.value.id == 'torch') \
                                else (fn.id if isinstance(fn, ast.Name) else None)
                            if name in ALLOC_CALLS and ch.name not in ('_ws', '_nhwc_out'):
                                found.add(mod + '.' + prefix + ch.name)
                                break
        visit(tree, '')
    return found, every


def test_every_allocating_entry_point_has_a_poisoned_case():
    import test_poisoned_memory_gpu as sweep
    found, every = allocating_functions()
    assert len(found) > 60, sorted(found)
    covered = set()
    for c in sweep.CASES:
        covered.update(c.entries)
    excluded = dict(sweep.EXCLUDED)
    assert all(isinstance(r, str) and len(r) > 20 for r in excluded.values())
    missing = sorted(found - covered - set(excluded))
    assert not missing, "allocating entry points with no poisoned case and no reasoned exclusion: %s" % missing
    assert not set(excluded) - found, "excluded entry points that do not allocate: %s" % sorted(set(excluded) - found)
    assert not covered - every, "case table names functions that do not exist (renamed?): %s" % sorted(covered - every)
    assert not covered & set(excluded), sorted(covered & set(excluded))
