"""CPU: tests/memguard.py itself -- poison fill, torch's own shapes and strides, band violations with their call site, the patch undone
on every exit, nested guards -- and the coverage check: every function of the package that allocates (found by reading every file of
the package, not a fixed list) has a case in tests/test_poisoned_memory_gpu.py or a reasoned exclusion, and nothing allocates by a
call the guard does not route."""
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


def test_a_nested_guard_joins_an_adopting_one(fake_module):
    """What the sweep relies on for test bodies that poison their own allocations: under an adopting guard an inner poisoned() routes
    to the outer guard and takes its pattern, and yields the inner block's own count, records and band check; without adopt= nothing
    changes."""
    with memguard.poisoned('B', modules=(), adopt=True) as outer:
        for asked in 'AB':
            with memguard.poisoned(asked, modules=('memguard_fake_mod',)) as inner:
                t = fake_module.alloc((4,), dtype=torch.int32)
                u = fake_module.alloc((2,), dtype=torch.float32)
                assert inner.count == 2 and len(inner.records) == 2 and inner.pattern == 'B'
            assert fake_module.torch is torch
            assert bool((memguard.bits(t) == 0x00).all()) and bool((memguard.bits(u) == 0x7F).all())
        assert outer.count == 4 and len(outer.records) == 4
        with pytest.raises(AssertionError, match="alloc"):
            with memguard.poisoned('A', modules=('memguard_fake_mod',)):
                t = fake_module.alloc((4,), dtype=torch.int32)
                _raw(t)[memguard.GUARD + 16] = 0
        _raw(t)[memguard.GUARD + 16] = memguard.GUARD_BYTE
    assert not memguard._ACTIVE and fake_module.torch is torch
    with memguard.poisoned('B', modules=()) as outer:
        with memguard.poisoned('A', modules=('memguard_fake_mod',)) as inner:
            t = fake_module.alloc((4,), dtype=torch.int32)
        assert inner is not outer and outer.count == 0 and inner.count == 1 and bool((memguard.bits(t) == 0xFF).all())
    assert not memguard._ACTIVE and fake_module.torch is torch


# ---------------------------------------------------------------- coverage of the allocating entry points
def allocating_functions():
    """({'module.qualname'} of every function / method of the package that allocates (memguard.scan_package), {'module.qualname'} of
    every function / method of the package), with the module's last name component as `module`, as the case table spells it."""
    every, found, _ = memguard.scan_package()
    short = {m: m.rsplit('.', 1)[-1] for m in found}
    assert len(set(short.values())) == len(short), "two allocating modules share a file name: %s" % sorted(short)
    names = set(short.values())
    flat_found = {short[m] + '.' + q for m, qs in found.items() for q in qs}
    flat_every = {m.rsplit('.', 1)[-1] + '.' + q for m, qs in every.items() if m in short or m.rsplit('.', 1)[-1] not in names for q in qs}
    return flat_found, flat_every


def test_the_guard_patches_every_allocating_module():
    import test_poisoned_memory_gpu as sweep
    _, found, _ = memguard.scan_package()
    assert len(found) >= 22, sorted(found)
    assert set(memguard.MODULES) | set(memguard.UNGUARDED) == set(found) and not set(memguard.MODULES) & set(memguard.UNGUARDED)
    assert {'upsnet_amd.ops', 'upsnet_amd.tta', 'upsnet_amd.group_norm', 'upsnet_amd.models.hipconv', 'upsnet_amd.dataset.pan_track',
            'upsnet_amd.dataset.mots'} <= set(memguard.MODULES)
    for m in memguard.UNGUARDED:        # left unpatched only where nothing of the module is swept
        names = {m.rsplit('.', 1)[-1] + '.' + q for q in found[m]}
        assert names <= set(sweep.EXCLUDED), "%s is not guarded, but not all of it is excluded: %s" % (m, sorted(names - set(sweep.EXCLUDED)))
    assert sorted(sweep._ENTRY_MODULES.values()) == sorted(memguard.MODULES)
    assert all(full.rsplit('.', 1)[-1] == short for short, full in sweep._ENTRY_MODULES.items())
    for m in memguard.MODULES:          # the patch replaces the module's global `torch`: a function-local import would escape it
        assert __import__(m, fromlist=['_']).__dict__.get('torch') is torch, "%s has no module-level `import torch`" % m


def test_no_uninitialised_allocation_escapes_the_proxy():
    """torch.empty_like, torch.empty_strided and Tensor.new_empty are not routed through the guard: the package must not call them."""
    calls = memguard.scan_package()[2]
    assert not calls, "uninitialised allocations that the guard does not route (use torch.empty): %s" % "; ".join(calls)


def test_the_scan_names_what_it_finds(tmp_path, monkeypatch):
    pkg = tmp_path / 'upsnet_amd' / 'sub'
    pkg.mkdir(parents=True)
    (tmp_path / 'upsnet_amd' / '__init__.py').write_text("")
    (pkg / 'mod.py').write_text(
        "import torch\n"
        "def _ws(n):\n    return torch.empty(n)\n"
        "def pinned(n):\n    return torch.empty(n, pin_memory=True)\n"
        "def plain(n):\n    return torch.zeros(n)\n"
        "class K:\n"
        "    def a(self, n):\n        return torch.empty((n,), device='cuda')\n"
        "    def b(self, n):\n        return _ws(n)\n"
        "    def c(self, x):\n        return torch.empty_like(x)\n"
        "def d(x):\n    y = x.new_empty((3,))\n    return torch.empty_strided((2,), (1,))\n"
        "def e(n, c, dev):\n    return ops._nhwc_out(n, c, 2, 2, dev)\n"
        "def f(n, dev):\n    return impl._ws(n, dev)\n"
        "def g(a):\n    return np.empty_like(a)\n"
        "class L:\n"
        "    def h(self):\n        return self._ws.numel()\n")
    monkeypatch.setattr(memguard, 'ROOT', str(tmp_path))
    every, found, unrouted = memguard.scan_package()
    assert found == {'upsnet_amd.sub.mod': {'K.a', 'K.b', 'e', 'f'}}      # (a helper called as an attribute counts; numpy's empty_like and a tensor
    # attribute named _ws do not)
    assert every == {'upsnet_amd.sub.mod': {'_ws', 'pinned', 'plain', 'K.a', 'K.b', 'K.c', 'd', 'e', 'f', 'g', 'L.h'}}
    rel = os.path.join('upsnet_amd', 'sub', 'mod.py')
    assert unrouted == [rel + ':14: torch.empty_like', rel + ':16: x.new_empty', rel + ':17: torch.empty_strided']


def test_every_allocating_entry_point_has_a_poisoned_case():
    import test_poisoned_memory_gpu as sweep
    found, every = allocating_functions()
    assert len(found) >= 102, sorted(found)
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
