"""CPU: the connected-component rule of upsnet_pan_components -- the two restatements of tests/pan_components_ref.py
against each other on every case of the GPU table and against hand-derived literals --, the configuration and command-line options,
the place where the evaluation applies it, and the argument checks of ops.pan_components that need no device."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import pan_components_ref as ref
from conftest import ROOT

K, S, V = (11, 1), (3, 0), (255, 0)


@pytest.fixture()
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    yield config
    config.clear()
    config.update(saved)


def build(rows, byte2=0):
    """uint8 [H,W,3] from rows of (category, instance) pairs."""
    pan = np.zeros((len(rows), len(rows[0]), 3), np.uint8)
    for y, row in enumerate(rows):
        for x, (c, i) in enumerate(row):
            pan[y, x] = (c, i, byte2)
    return pan


def both(pan, *a):
    f, s = ref.clean_flood(pan, *a), ref.clean_scipy(pan, *a)
    for x, y in zip(f, s):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    return f


def test_the_tile_of_the_case_table_is_the_kernels():
    src = open(os.path.join(ROOT, 'upsnet_amd', 'csrc', 'pan_components.hip')).read()
    assert int(re.search(r'#define PC_TH (\d+)', src).group(1)) == ref.TH
    assert int(re.search(r'#define PC_TW (\d+)', src).group(1)) == ref.TW


def test_the_two_restatements_agree_on_the_gpu_table():
    names = []
    for name, pan, min_area, keep in ref.cases():
        names.append(name)
        for conn in (4, 8):
            out, labels, stats = both(pan, min_area, conn, keep)
            assert out.shape == pan.shape and labels.shape == pan.shape[:2] and stats.shape == (4,), name
            assert np.array_equal(out[..., 2], pan[..., 2]), name
            void = pan[..., 0] == 255
            assert np.array_equal(out[void], pan[void]) and bool((labels[void] == -1).all()) and bool((labels[~void] >= 0).all()), name
            assert stats[3] == int((out != pan).any(-1).sum()) == int((out[..., 0] != pan[..., 0]).sum()), name
    assert len(set(names)) == len(names) and 'full_1024x2048' in names


def test_table_cases_do_what_their_names_say():
    table = {name: (pan, m, k) for name, pan, m, k in ref.cases(full_size=False)}
    H, W = table['checkerboard'][0].shape[:2]
    assert both(table['checkerboard'][0], 0, 4, True)[2].tolist() == [2, H * W, 0, 0]          # every pixel its own component
    assert both(table['checkerboard'][0], 0, 8, True)[2].tolist() == [2, 2, 0, 0]              # two, across every seam
    assert both(table['checkerboard'][0], 2, 4, True)[2].tolist() == [2, H * W, H * W - 2, H * W - 2]
    pan = table['serpentine'][0]
    assert pan.shape[0] >= 3 * ref.TH and pan.shape[1] >= 3 * ref.TW
    for conn in (4, 8):
        _, labels, _ = both(pan, 0, conn, True)
        assert bool((labels[pan[..., 0] == 11] == 0).all())                                    # one chain from the first pixel
    for conn in (4, 8):
        _, labels, stats = both(table['u_shape'][0], 0, conn, True)
        assert stats.tolist()[:2] == [1, 1] and labels[9, 100] == 5 * 200 + 100                # the lower arm joins the upper one
    for name, axis, seam in (('comb', 0, ref.TH), ('comb_transposed', 1, ref.TW)):
        pan = table[name][0] if axis == 0 else table[name][0].transpose(1, 0, 2)     # teeth along axis 0, the seam at row `seam`
        assert pan.shape[0] > seam + 8 and pan.shape[1] >= 60
        teeth = pan[seam - 7:seam + 8, :, 0] == 11
        cols = np.flatnonzero(teeth.all(0))                             # every tooth lies on both sides of the seam
        assert len(cols) >= 30 and not teeth[:, [c for c in range(pan.shape[1]) if c not in cols]].any()
        assert bool((pan[seam - 1, cols, 0] == 11).all()) and bool((pan[seam, cols, 0] == 11).all())
        assert bool((pan[seam + 8, :, 0] == 11).all()) and not (pan[:seam - 7, :, 0] == 11).any()   # they meet only in the spine
        for conn in (4, 8):
            _, labels, _ = both(table[name][0], 0, conn, True)
            assert len(np.unique(labels[table[name][0][..., 0] == 11])) == 1
    pan = table['corner'][0]
    assert both(pan, 0, 8, True)[2].tolist() == [2, 2, 0, 0] and both(pan, 0, 4, True)[2].tolist() == [2, 4, 0, 0]
    assert both(pan, 2, 8, False)[2].tolist() == [2, 2, 0, 0] and both(pan, 2, 4, False)[2].tolist() == [2, 4, 4, 4]
    pan, m, _ = table['thresholds']
    assert m == 5 and both(pan, m, 4, True)[2].tolist()[2:] == [1, 4]                           # only the fragment of min_area - 1 goes
    pan, m, _ = table['tie']
    out, labels, stats = both(pan, m, 8, True)
    assert stats.tolist() == [1, 3, 2, 17] and out[3, 2, 0] == 11 and out[30, 10, 0] == 255    # equal areas: the smaller label stays
    pan = table['many_instances'][0]
    assert both(pan, 0, 8, True)[2][0] >= 256 and len(np.unique(pan[pan[..., 0] == 11][:, 1])) == 255
    assert both(table['all_void'][0], 5, 8, True)[2].tolist() == [0, 0, 0, 0]
    assert both(table['random_131x257'][0], 0, 4, True)[2][1] > 5000


BODY = [
    [K, K, K, S, S, S, S],
    [K, K, K, S, S, S, S],
    [K, K, K, S, S, K, K],
    [S, S, S, K, S, S, S],
    [S, S, S, S, S, S, S],
]


def test_hand_derived_island_and_diagonal_neighbour():
    """5 x 7: a 3 x 3 body, a pixel at (3, 3) that touches it only diagonally, a 2-pixel island at (2, 5..6); min_area 3."""
    pan = build(BODY, byte2=9)
    out, labels, stats = both(pan, 3, 8, True)
    want = [row[:] for row in BODY]
    want[2][5] = want[2][6] = V
    assert np.array_equal(out, build(want, byte2=9)) and stats.tolist() == [2, 3, 1, 2]
    assert labels.tolist() == [[0, 0, 0, 3, 3, 3, 3],
                               [0, 0, 0, 3, 3, 3, 3],
                               [0, 0, 0, 3, 3, 19, 19],
                               [3, 3, 3, 0, 3, 3, 3],
                               [3, 3, 3, 3, 3, 3, 3]]
    out, labels, stats = both(pan, 3, 4, True)
    want[3][3] = V                                                     # under 4-connectivity the diagonal neighbour is alone
    assert np.array_equal(out, build(want, byte2=9)) and stats.tolist() == [2, 4, 2, 3]
    assert labels[3, 3] == 24 and labels[2, 5] == 19 and labels[4, 6] == 3
    out, _, stats = both(pan, 0, 4, True)
    assert np.array_equal(out, pan) and stats.tolist() == [2, 4, 0, 0]


def test_hand_derived_tie_and_keep_largest_off():
    pan = build([[K, K, V, K, K, V, K, V, V]])
    out, labels, stats = both(pan, 5, 8, True)
    assert np.array_equal(out, build([[K, K, V, V, V, V, V, V, V]])) and stats.tolist() == [1, 3, 2, 3]
    assert labels.tolist() == [[0, 0, -1, 3, 3, -1, 6, -1, -1]]
    out, _, stats = both(pan, 5, 8, False)                             # the whole segment goes
    assert np.array_equal(out, build([[V] * 9])) and stats.tolist() == [1, 3, 3, 5]
    out, _, stats = both(pan, 2, 4, False)
    assert np.array_equal(out, build([[K, K, V, K, K, V, V, V, V]])) and stats.tolist() == [1, 3, 1, 1]


def test_hand_derived_void_and_byte_2_are_left_alone():
    pan = np.array([[(255, 9, 77), (11, 1, 42), (255, 3, 1), (3, 0, 5)]], np.uint8)
    out, labels, stats = both(pan, 2, 8, False)
    assert out.tolist() == [[[255, 9, 77], [255, 0, 42], [255, 3, 1], [255, 0, 5]]]
    assert labels.tolist() == [[-1, 1, -1, 3]] and stats.tolist() == [2, 2, 2, 2]
    out, _, stats = both(pan, 2, 8, True)
    assert np.array_equal(out, pan) and stats.tolist() == [2, 2, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- configuration
def test_config_defaults(saved_config):
    assert saved_config.test.pan_min_component == 0 and saved_config.test.pan_component_connectivity == 8
    assert saved_config.test.pan_component_keep_largest is True


def test_cli_options_set_the_config(saved_config, capsys):
    from upsnet_amd.config.parse_args import parse_args
    args = parse_args('t', [])
    assert args.pan_min_component is None and args.pan_component_connectivity is None and saved_config.test.pan_min_component == 0
    parse_args('t', ['--pan_min_component', '64'])
    assert saved_config.test.pan_min_component == 64 and saved_config.test.pan_component_connectivity == 8
    parse_args('t', ['--pan_min_component', '32', '--pan_component_connectivity', '4'])
    assert saved_config.test.pan_min_component == 32 and saved_config.test.pan_component_connectivity == 4
    saved_config.test.pan_min_component = 0
    for argv, option in ((['--pan_component_connectivity', '4'], '--pan_component_connectivity'),       # without its parent
                         (['--pan_min_component', '8', '--pan_component_connectivity', '6'], '--pan_component_connectivity'),
                         (['--pan_min_component', '-1'], '--pan_min_component'),
                         (['--pan_min_component', 'many'], '--pan_min_component')):
        saved_config.test.pan_min_component = 0
        capsys.readouterr()
        with pytest.raises(SystemExit):
            parse_args('t', argv)
        assert option in capsys.readouterr().err, argv
    assert 'which is missing' in _error_of(parse_args, ['--pan_component_connectivity', '8'], capsys, saved_config)


def _error_of(parse_args, argv, capsys, cfg):
    cfg.test.pan_min_component = 0
    capsys.readouterr()
    with pytest.raises(SystemExit):
        parse_args('t', argv)
    return capsys.readouterr().err


def test_yaml_keys_set_the_config(tmp_path, saved_config):
    from test_dataset_run_cpu import write_cfg
    from upsnet_amd.config.parse_args import parse_args
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val', extra='  pan_min_component: 50\n  pan_component_keep_largest: false\n')
    parse_args('t', ['--cfg', cfg, '--pan_component_connectivity', '4'])     # the yaml switched it on
    assert saved_config.test.pan_min_component == 50 and saved_config.test.pan_component_connectivity == 4
    assert saved_config.test.pan_component_keep_largest is False


@pytest.mark.parametrize('extra,key', [('  pan_min_component: 50\n  pan_component_connectivity: 6\n', 'test.pan_component_connectivity'),
                                       ('  pan_min_component: -3\n', 'test.pan_min_component'),
                                       ('  pan_min_component: 2.5\n', 'test.pan_min_component'),
                                       ('  pan_min_component: 5\n  pan_component_keep_largest: 3\n', 'test.pan_component_keep_largest')])
def test_bad_yaml_values_end_at_parse_time_naming_the_key(tmp_path, saved_config, capsys, extra, key):
    from test_dataset_run_cpu import write_cfg
    from upsnet_amd import sequence
    from upsnet_amd.config.parse_args import parse_args
    cfg = write_cfg(tmp_path, 'Cityscapes', str(tmp_path / 'data'), 'val', extra=extra)
    with pytest.raises(SystemExit):
        parse_args('t', ['--cfg', cfg])
    assert key in capsys.readouterr().err
    cats = tmp_path / 'cats.json'
    cats.write_text('{"categories": []}')
    with pytest.raises(SystemExit, match=key):                            # the sequence command line: the same check, the same words
        sequence.main(['--cfg', cfg, '--track_only', str(tmp_path), '--out', str(tmp_path / 'o'), '--panoptic_categories', str(cats)])


def test_sequence_command_line_takes_the_options():
    from upsnet_amd.sequence import parse_args
    args = parse_args(['--cfg', 'x.yaml', '--track_only', 'f', '--out', 'o', '--pan_min_component', '40', '--pan_component_connectivity', '4'])
    assert args.pan_min_component == 40 and args.pan_component_connectivity == 4
    assert parse_args(['--cfg', 'x.yaml']).pan_min_component is None


class FakeDataset(object):
    def __init__(self):
        self.cleaned = []

    def __len__(self):
        return 2

    def get_unified_pan_result(self, segs, pans, cls_inds, stuff_area_limit):
        return ['unified', segs, pans, cls_inds, stuff_area_limit]

    def get_combined_pan_result(self, segs, boxes, masks, stuff_area_limit):
        return ['combined', segs, boxes, masks, stuff_area_limit]

    def clean_pan_result(self, pans, **kw):
        self.cleaned.append((pans, kw))
        return ['cleaned', pans]


def test_panoptic_predictions_cleans_only_when_asked(saved_config):
    from upsnet_amd.evaluate import panoptic_predictions
    results = {'all_ssegs': ['s0', 's1'], 'all_panos': ['p0', 'p1'], 'all_pano_cls_inds': ['c0', 'c1'],
               'all_boxes': [[], ['b0', 'b1']], 'all_masks': [[], ['m0', 'm1']]}
    limit = saved_config.test.panoptic_stuff_area_limit
    unified = ['unified', ['s1', 's0'], ['p1', 'p0'], ['c1', 'c0'], limit]
    combined = ['combined', ['s0', 's1'], [[], ['b0', 'b1']], [[], ['m0', 'm1']], limit]
    ds = FakeDataset()
    assert saved_config.test.pan_min_component == 0
    assert panoptic_predictions(ds, results, False, [1, 0]) == unified             # what it returned before the option existed
    assert panoptic_predictions(ds, results, True) == combined
    assert ds.cleaned == []
    saved_config.test.pan_min_component = 7
    assert panoptic_predictions(ds, results, False, [1, 0]) == ['cleaned', unified]
    assert panoptic_predictions(ds, results, True) == ['cleaned', combined]
    assert [p for p, _ in ds.cleaned] == [unified, combined]


def test_clean_panoptic_is_exported_and_checks_its_arguments():
    from upsnet_amd.dataset import clean_panoptic
    from upsnet_amd.dataset.base_dataset import BaseDataset
    assert callable(BaseDataset.clean_pan_result)
    pan = np.zeros((4, 5, 3), np.uint8)
    for bad in (dict(min_area=-1), dict(min_area=2.5), dict(min_area=3, connectivity=6)):
        with pytest.raises(ValueError):
            clean_panoptic([pan], **bad)
    with pytest.raises(ValueError):
        clean_panoptic([np.zeros((4, 5), np.uint8)], 3)
    with pytest.raises(ValueError):
        clean_panoptic([np.zeros((0, 5, 3), np.uint8)], 3)
    assert clean_panoptic([], 3) == []


def test_ops_argument_checks_that_need_no_device():
    from upsnet_amd import ops
    good = torch.zeros((4, 5, 3), dtype=torch.uint8)
    for bad in (torch.zeros((4, 5, 3), dtype=torch.int32), torch.zeros((4, 5), dtype=torch.uint8), torch.zeros((4, 5, 2), dtype=torch.uint8),
                torch.zeros((5, 4, 3), dtype=torch.uint8).permute(1, 0, 2), torch.zeros((0, 5, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError, match='pan_components'):
            ops.pan_components(bad)
    for kw in (dict(connectivity=6), dict(connectivity=0), dict(min_area=-1), dict(min_area=1.5), dict(min_area=True),
               dict(out=torch.zeros((4, 4, 3), dtype=torch.uint8)), dict(labels=torch.zeros((4, 5), dtype=torch.int64)),
               dict(labels=torch.zeros((5, 4), dtype=torch.int32))):
        with pytest.raises(ValueError, match='pan_components'):
            ops.pan_components(good, **kw)
    with pytest.raises(ValueError, match='2\\^24'):
        ops.pan_components_workspace(4097, 4096, 'cpu')
    with pytest.raises(Exception, match='not implemented'):                  # a host tensor: there is no CPU path
        ops.pan_components(good)
    from upsnet_amd._lib import lib
    assert lib().upsnet_pan_components_workspace_bytes(0, 5) == 0 and lib().upsnet_pan_components_workspace_bytes(4096, 4097) == 0
    assert lib().upsnet_pan_components_workspace_bytes(4096, 4096) == 65536 * 8 + 2 * 4 * (1 << 24)
    one = lib().upsnet_pan_components_workspace_bytes(1, 1)
    assert one == 65536 * 8 + 16 + 4
    # the C entry point refuses bad arguments before any launch (no device is touched: this runs without one)
    from ctypes import c_void_p
    p = c_void_p(1 << 20)
    assert lib().upsnet_pan_components(None, None, 4, 5, 8, 0, 1, p, p, None, p) != 0 and b'null pointer' in lib().upsnet_last_error()
    assert lib().upsnet_pan_components(None, p, 4096, 4097, 8, 0, 1, p, p, None, p) != 0 and b'2^24' in lib().upsnet_last_error()
    assert lib().upsnet_pan_components(None, p, 4, 5, 6, 0, 1, p, p, None, p) != 0 and b'connectivity 6' in lib().upsnet_last_error()
    assert lib().upsnet_pan_components(None, p, 4, 5, 4, -3, 1, p, p, None, p) != 0 and b'min_area -3' in lib().upsnet_last_error()
    assert lib().upsnet_pan_components(None, p, 4, 5, 4, 3, 1, c_void_p((1 << 20) + 4), p, None, p) != 0 and b'aligned' in lib().upsnet_last_error()
