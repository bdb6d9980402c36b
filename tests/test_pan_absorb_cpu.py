"""CPU: the absorbing rule of upsnet_pan_absorb -- the two restatements of tests/pan_absorb_ref.py against each other on
every case of the GPU table, against hand-derived literals and against the properties the rule implies --, the configuration and
command-line option, and the argument checks that need no device."""
import copy

import numpy as np
import pytest
import torch

import pan_absorb_ref as aref
import pan_components_ref as ref

ALL_CASES = ref.cases() + aref.cases()


@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def both(pan, *a):
    v = aref.absorb_vec(pan, *a)
    if pan.shape[0] * pan.shape[1] <= aref.LOOP_MAX_PIXELS:
        for x, y in zip(aref.absorb_loop(pan, *a), v):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
    return v


def test_case_names_are_unique_and_the_table_holds_what_it_promises():
    names = [c[0] for c in ALL_CASES]
    assert len(set(names)) == len(names) and 'full_1024x2048' in names
    table = {c[0]: c for c in aref.cases()}
    assert table['absorb_1x1'][1].shape[:2] == (1, 1) and table['absorb_1x40'][1].shape[:2] == (1, 40)
    assert table['absorb_40x1'][1].shape[:2] == (40, 1)
    for name in ('absorb_33x129', 'absorb_70x300'):
        H, W = table[name][1].shape[:2]
        assert H > ref.TH and W > ref.TW and H % ref.TH and W % ref.TW
    _, pan, m, keep = table['seam_cross']                               # one fragment in all four tiles, donors in all four too
    out, labels, stats = both(pan, m, 8, keep)
    frag = out[..., 0] != pan[..., 0]
    assert stats.tolist()[2:7] == [1, 76, 1, 76, 4]
    assert all(bool(frag[ys, xs].any()) for ys in (np.s_[:ref.TH], np.s_[ref.TH:]) for xs in (np.s_[:ref.TW], np.s_[ref.TW:]))
    _, pan, m, keep = table['corners']
    out, _, stats = both(pan, m, 8, keep)
    assert stats.tolist()[2:6] == [4, 10, 4, 10]
    assert all(tuple(out[y, x, :2]) == (3, 0) and tuple(pan[y, x, :2]) == (11, 7) for y in (0, 39) for x in (0, 149))
    _, pan, m, keep = table['long_fragment']
    out, _, stats = both(pan, m, 8, keep)
    # columns 5..204 lie under the stripes 1..68: 68 keys of at most 3 votes, and (3, 0) with 200 from below and one from either end
    assert stats.tolist()[2:7] == [1, 200, 1, 200, 69] and bool((out[5, 5:205, :2] == (3, 0)).all())
    _, pan, m, keep = table['stripes']
    H, W = pan.shape[:2]
    for conn in (4, 8):
        stats = both(pan, m, conn, keep)[2]
        assert stats[2] == stats[3] == H * W // 2 - 2 and stats[4] == stats[2]
        # every edge of the map joins a fragment pixel and a kept pixel of a key of its own, but for the three edges each of the two
        # fragment-key pixels that are kept as main components
        assert stats[6] == 2 * H * W - H - W - 6
    assert len(np.unique(table['many_instances_cells'][1][..., 1])) == 256


@pytest.mark.parametrize('case', ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_restatements_agree_and_the_properties_hold(case):
    name, pan, min_area, keep = case
    big = pan.shape[0] * pan.shape[1] > aref.LOOP_MAX_PIXELS
    for conn in ((8,) if big else (4, 8)):
        void = (ref.clean_scipy if big else ref.clean_flood)(pan, min_area, conn, keep)
        out, labels, stats = aref.absorb_vec(pan, min_area, conn, keep, base=void) if big else both(pan, min_area, conn, keep)
        assert out.dtype == np.uint8 and out.shape == pan.shape and labels.dtype == np.int32 and stats.dtype == np.int32
        assert stats.shape == (8,) and stats[:4].tolist() == void[2].tolist() and stats[7] == 0
        assert np.array_equal(labels, void[1]) and np.array_equal(out[..., 2], pan[..., 2])
        # the output differs from the void mode's exactly on the absorbed pixels, which were fragment pixels and are not VOID now
        differs = (out != void[0]).any(-1)
        assert int(differs.sum()) == stats[5] and bool((void[0][differs][:, 0] == 255).all()) and bool((out[differs][:, 0] != 255).all())
        assert bool((pan[differs][:, 0] != 255).all()) and stats[4] <= stats[2] and stats[4] <= stats[6]
        # min_area == 0 is the identity
        if not big:
            same, _, s0 = aref.absorb_vec(pan, 0, conn, keep)
            assert np.array_equal(same, pan) and s0[2:].tolist() == [0] * 6
        # a fixed point: a second application removes nothing
        again, _, s2 = aref.absorb_vec(out, min_area, conn, keep)
        assert np.array_equal(again, out) and s2[2:].tolist() == [0] * 6, name


@pytest.mark.parametrize('literal', aref.literals(), ids=[l[0] for l in aref.literals()])
def test_hand_derived_literals(literal):
    name, rows, min_area, keep, want_rows, want_stats = literal
    pan = aref.build(rows, byte2=9)
    for conn in (4, 8):
        out, labels, stats = both(pan, min_area, conn, keep)
        assert np.array_equal(out, aref.build(want_rows, byte2=9)), (name, conn)
        assert stats.tolist() == want_stats, (name, conn)
        assert np.array_equal(labels, ref.clean_flood(pan, min_area, conn, keep)[1])


def test_diagonal_only_differs_from_an_edge():
    """The same map with the fragment moved one pixel up touches S along an edge and is absorbed."""
    rows = [row[:] for row in next(l for l in aref.literals() if l[0] == 'diagonal_only')[1]]
    rows[2][2], rows[1][2] = aref.V, aref.K7
    out, _, stats = both(aref.build(rows), 2, 8, True)
    assert tuple(out[1, 2, :2]) == aref.S and stats.tolist()[2:] == [1, 1, 1, 1, 1, 0]


# ---------------------------------------------------------------------------------------------------------------- configuration
def test_config_default(saved_config):
    assert saved_config.test.pan_component_mode == 'void'


def _error_of(parse_args, argv, capsys, cfg):
    cfg.test.pan_min_component = 0
    capsys.readouterr()
    with pytest.raises(SystemExit):
        parse_args('t', argv)
    return capsys.readouterr().err


def test_cli_option_sets_the_config(saved_config, capsys):
    from upsnet_amd.config.parse_args import parse_args
    args = parse_args('t', [])
    assert args.pan_component_mode is None and saved_config.test.pan_component_mode == 'void'
    parse_args('t', ['--pan_min_component', '64'])
    assert saved_config.test.pan_component_mode == 'void'
    parse_args('t', ['--pan_min_component', '64', '--pan_component_mode', 'absorb'])
    assert saved_config.test.pan_min_component == 64 and saved_config.test.pan_component_mode == 'absorb'
    parse_args('t', ['--pan_min_component', '64', '--pan_component_mode', 'void'])
    assert saved_config.test.pan_component_mode == 'void'
    err = _error_of(parse_args, ['--pan_component_mode', 'absorb'], capsys, saved_config)                 # without its parent
    sibling = _error_of(parse_args, ['--pan_component_connectivity', '8'], capsys, saved_config)
    assert '--pan_component_mode is a parameter of --pan_min_component, which is missing' in err
    last = lambda text: text.strip().splitlines()[-1]
    assert last(err).replace('--pan_component_mode', '--pan_component_connectivity') == last(sibling)     # its sibling's message
    err = _error_of(parse_args, ['--pan_min_component', '8', '--pan_component_mode', 'fill'], capsys, saved_config)
    assert '--pan_component_mode' in err and 'fill' in err


def test_yaml_key_sets_the_config_and_is_checked(tmp_path, saved_config, capsys):
    from test_dataset_run_cpu import write_cfg
    from upsnet_amd import sequence
    from upsnet_amd.config.parse_args import parse_args
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val', extra='  pan_min_component: 50\n  pan_component_mode: absorb\n')
    parse_args('t', ['--cfg', cfg])
    assert saved_config.test.pan_min_component == 50 and saved_config.test.pan_component_mode == 'absorb'
    parse_args('t', ['--cfg', cfg, '--pan_component_mode', 'void'])             # the yaml switched the cleaning on; the option wins
    assert saved_config.test.pan_component_mode == 'void'
    bad = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val', name='bad.yaml',
                    extra='  pan_min_component: 50\n  pan_component_mode: fill\n')
    with pytest.raises(SystemExit):
        parse_args('t', ['--cfg', bad])
    assert 'test.pan_component_mode' in capsys.readouterr().err
    cats = tmp_path / 'cats.json'
    cats.write_text('{"categories": []}')
    with pytest.raises(SystemExit, match='test.pan_component_mode'):       # the sequence command line: the same check, the same words
        sequence.main(['--cfg', bad, '--track_only', str(tmp_path), '--out', str(tmp_path / 'o'), '--panoptic_categories', str(cats)])


def test_sequence_command_line_takes_the_option():
    from upsnet_amd.sequence import parse_args
    args = parse_args(['--cfg', 'x.yaml', '--track_only', 'f', '--out', 'o', '--pan_min_component', '40', '--pan_component_mode', 'absorb'])
    assert args.pan_min_component == 40 and args.pan_component_mode == 'absorb'
    assert parse_args(['--cfg', 'x.yaml']).pan_component_mode is None


class Recorder(object):
    def __init__(self):
        self.calls = []

    def __call__(self, pans, *a, **kw):
        self.calls.append((a, kw))
        return list(pans), None


def test_clean_pan_result_takes_the_mode_from_the_config(saved_config, monkeypatch):
    from upsnet_amd.dataset import pan_components
    from upsnet_amd.dataset.base_dataset import BaseDataset
    rec = Recorder()
    monkeypatch.setattr(pan_components, 'clean_panoptic', rec)
    saved_config.test.pan_min_component = 5
    BaseDataset().clean_pan_result([])
    saved_config.test.pan_component_mode = 'absorb'
    BaseDataset().clean_pan_result([])
    BaseDataset().clean_pan_result([], mode='void')
    assert [kw['mode'] for _, kw in rec.calls] == ['void', 'absorb', 'void']


# ---------------------------------------------------------------------------------------------------------------- argument checks
def test_clean_panoptic_refuses_an_unknown_mode():
    from upsnet_amd.dataset import clean_panoptic
    pan = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(ValueError, match='nonsense'):
        clean_panoptic([pan], 3, mode='nonsense')
    with pytest.raises(ValueError, match='nonsense'):
        clean_panoptic([], 3, mode='nonsense')
    for mode in ('void', 'absorb'):
        assert clean_panoptic([], 3, mode=mode) == []
        with pytest.raises(ValueError):
            clean_panoptic([pan], -1, mode=mode)


def test_ops_argument_checks_that_need_no_device():
    from upsnet_amd import ops
    good = torch.zeros((4, 5, 3), dtype=torch.uint8)
    for bad in (torch.zeros((4, 5, 3), dtype=torch.int32), torch.zeros((4, 5), dtype=torch.uint8), torch.zeros((4, 5, 2), dtype=torch.uint8),
                torch.zeros((5, 4, 3), dtype=torch.uint8).permute(1, 0, 2), torch.zeros((0, 5, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError, match='pan_absorb'):
            ops.pan_absorb(bad)
    for kw in (dict(connectivity=6), dict(connectivity=0), dict(min_area=-1), dict(min_area=1.5), dict(min_area=True),
               dict(out=torch.zeros((4, 4, 3), dtype=torch.uint8)), dict(labels=torch.zeros((4, 5), dtype=torch.int64)),
               dict(labels=torch.zeros((5, 4), dtype=torch.int32))):
        with pytest.raises(ValueError, match='pan_absorb'):
            ops.pan_absorb(good, **kw)
    with pytest.raises(ValueError, match='2\\^24'):
        ops.pan_absorb_workspace(4097, 4096, 'cpu')
    with pytest.raises(Exception, match='not implemented'):                  # a host tensor: there is no CPU path
        ops.pan_absorb(good)


def test_c_entry_point_sizes_and_refusals():
    from ctypes import c_void_p
    from upsnet_amd._lib import lib
    size, base = lib().upsnet_pan_absorb_workspace_bytes, lib().upsnet_pan_components_workspace_bytes
    assert size(0, 5) == 0 and size(4096, 4097) == 0 and size(5, -1) == 0
    # best | parent | area as upsnet_pan_components, then a 64-bit winner per pixel and 2 H W slots of 8 + 4 bytes, each part padded to 16
    pad = lambda n: (n + 15) // 16 * 16
    for H, W in ((1, 1), (3, 7), (37, 53), (1024, 2048), (4096, 4096)):
        n = H * W
        assert size(H, W) == pad(base(H, W)) + pad(8 * n) + 16 * n + pad(8 * n), (H, W)
    # the entry point refuses bad arguments before any launch (no device is touched: this runs without one), in pan_components' words
    p = c_void_p(1 << 20)
    f, err = lib().upsnet_pan_absorb, lib().upsnet_last_error
    assert f(None, None, 4, 5, 8, 0, 1, p, p, None, p) != 0 and err() == b'pan_absorb: null pointer'
    assert f(None, p, 4, 5, 8, 0, 1, p, p, None, None) != 0 and err() == b'pan_absorb: null pointer'
    assert f(None, p, 4096, 4097, 8, 0, 1, p, p, None, p) != 0 and err().startswith(b'pan_absorb: ') and b'2^24' in err()
    assert f(None, p, 4, 5, 6, 0, 1, p, p, None, p) != 0 and err() == b'pan_absorb: connectivity 6 is neither 4 nor 8'
    assert f(None, p, 4, 5, 4, -3, 1, p, p, None, p) != 0 and err() == b'pan_absorb: min_area -3 is negative'
    assert f(None, p, 4, 5, 4, 3, 1, c_void_p((1 << 20) + 4), p, None, p) != 0 and err().startswith(b'pan_absorb: ') and b'aligned' in err()
    g = lib().upsnet_pan_components                                          # and pan_components keeps its own words
    assert g(None, p, 4, 5, 6, 0, 1, p, p, None, p) != 0 and err() == b'pan_components: connectivity 6 is neither 4 nor 8'
