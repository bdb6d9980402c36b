"""GPU: the panoptic confidence through the model and the files, synthetic weights on a 128 x 256 image (the smallest
the suite runs the model on). With config.test.pan_confidence the label maps are bit-equal to a run without it; the plane of the graph
replay equals the eager one; the plain-torch plane of the paths without the kernel agrees with it within one step of the byte; without
the planes write_panoptic's files are byte for byte what they were, with them every segment gains "score" and nothing else changes."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pan_confidence_ref as ref  # noqa: E402
from conftest import gen_panoptic_maps  # noqa: E402
from oracle import ops as oops  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def saved_config():
    from upsnet_amd.config.config import config
    saved = copy.deepcopy(dict(config))
    try:
        yield config
    finally:
        config.clear()
        config.update(saved)


@pytest.fixture(scope="module")
def setup():
    from upsnet_amd.config.config import config, update_config_dict, CITYSCAPES_R50
    saved = copy.deepcopy(dict(config))
    update_config_dict(CITYSCAPES_R50)
    from upsnet_amd.synthetic import build_model, make_image
    model, data = build_model(), make_image(128, 256, seed=3, device='cuda')
    was = model.use_graph
    model.use_graph = False
    with torch.no_grad():
        base = {k: v.clone() for k, v in model(data).items()}
    yield model, data, base
    model.use_graph = was
    config.clear()
    config.update(saved)


def test_option_off_adds_nothing(setup):
    assert 'panoptic_conf' not in setup[2]


def test_eager_labels_unchanged_and_graph_replay_equal(setup, saved_config):
    model, data, base = setup
    saved_config.test.pan_confidence = True
    with torch.no_grad():
        model.use_graph = False
        on = {k: v.clone() for k, v in model(data).items()}
        assert set(on) == set(base) | {'panoptic_conf'}
        for k in base:
            assert torch.equal(on[k], base[k]), k
        conf = on['panoptic_conf']
        assert conf.dtype == torch.uint8 and conf.shape == on['panoptic_outputs'].shape
        assert int(conf.min()) >= 1 and len(torch.unique(conf)) > 16          # a real plane: P[winner] >= 1 / channels, and it varies
        was = (model.use_graph, model.graph_slots)
        try:
            model.use_graph, model.graph_slots = True, 1
            for _ in range(4):               # two eager forwards, the capture, a replay
                g = {k: v.clone() for k, v in model(data).items()}
            slots = [s for key, v in model._graphs.items() if key[-1] == 'conf' for s in v['slots']]
            assert slots and all('graph' in s for s in slots), "the forward with the confidence plane was not captured"
            assert 'conf' in slots[0]['out']['tail']
        finally:
            model.use_graph, model.graph_slots = was
        assert torch.equal(g['panoptic_conf'], conf)
        assert torch.equal(g['panoptic_outputs'], base['panoptic_outputs']) and torch.equal(g['fcn_outputs'], base['fcn_outputs'])
    # pan_min_score alone asks for the plane too
    saved_config.test.pan_confidence, saved_config.test.pan_min_score = False, 0.25
    model.use_graph = False
    with torch.no_grad():
        assert torch.equal(model(data)['panoptic_conf'], conf)


def test_torch_fallback_agrees_within_one_step(setup, saved_config):
    """The path of n_pan > 256 (materialised planes, plain torch) on an image the kernel serves too; torch's upsampling and exp are not
    the kernel's, so the bytes may differ by one."""
    model, data, base = setup
    saved_config.test.pan_confidence = True
    model.use_graph = False
    model.taps = {}
    try:
        with torch.no_grad():
            out = model(data)
            t = model.taps
            fcn_output = F.interpolate(t['fcn_score'], None, 4, mode='bilinear', align_corners=False)
            H, W = fcn_output.shape[2:]
            keep, num_keep, real_keep = model.mask_removal.select(t['pan_boxes'][:, 1:], t['pan_scores'], t['pan_logit'], t['pan_cls'], (H, W))
            pan, sem, conf = model._materialised_head(fcn_output, t['pan_boxes'], t['pan_logit'], t['pan_cls'], keep, num_keep, real_keep, True)
    finally:
        model.taps = None
    assert conf.dtype == torch.uint8 and conf.shape == out['panoptic_conf'].shape
    step = (conf.int() - out['panoptic_conf'].int()).abs().max().item()
    print("fallback vs kernel: max |dq| = %d; labels differ on %d pixels" % (step, int((pan != out['panoptic_outputs']).sum())))
    assert step <= 1
    # the module-level forward has the key as well
    model.pipeline = 'modules'
    try:
        with torch.no_grad():
            mod = model(data)
    finally:
        model.pipeline = 'fused'
    assert mod['panoptic_conf'].dtype == torch.uint8 and mod['panoptic_conf'].shape == mod['panoptic_outputs'].shape


# ---------------------------------------------------------------------------------------------------------------------------- files
CATS = [{'id': c, 'name': 'c%d' % c, 'isthing': int(c > 10), 'color': [10 * c + 5, 255 - 9 * c, (37 * c) % 256]} for c in range(19)]


def _maps():
    out = []
    for s, (H, W) in enumerate([(64, 96), (80, 120)]):
        rng = np.random.default_rng(50 + s)
        seg, pan, cls = gen_panoptic_maps(rng, H, W, 7)
        out.append((oops.get_unified_pan_result(seg, pan, cls, 19, 9, 200), rng.integers(0, 256, (H, W)).astype(np.uint8)))
    return out


def _tree(folder):
    files = {}
    for d, _, names in os.walk(folder):
        for n in names:
            with open(os.path.join(d, n), 'rb') as f:
                files[os.path.relpath(os.path.join(d, n), folder)] = f.read()
    return files


def test_write_panoptic_files(tmp_path):
    from upsnet_amd.dataset.pan_format import panoptic_format, write_panoptic
    from upsnet_amd.dataset.pan_confidence import filter_by_score, segment_scores
    maps = _maps()
    pans = [torch.from_numpy(p).cuda() for p, _ in maps]
    confs = [c for _, c in maps]
    images = [{'id': 7 + i, 'file_name': 'im%d.jpg' % i} for i in range(len(maps))]
    # without the planes: the annotations are panoptic_format's, the JSON is their plain dump, as before the option existed
    plain = write_panoptic(pans, images, CATS, str(tmp_path / 'plain'))
    want = [{'image_id': im['id'], 'file_name': 'im%d.png' % i, 'segments_info': panoptic_format(p, CATS)[1]}
            for i, (im, p) in enumerate(zip(images, pans))]
    assert plain == want and all('score' not in s for a in plain for s in a['segments_info'])
    files = _tree(str(tmp_path / 'plain'))
    assert sorted(files) == ['pan/im0.png', 'pan/im1.png', 'pan_2ch/im0.png', 'pan_2ch/im1.png', 'pred.json']
    assert files['pred.json'] == json.dumps({'annotations': want}).encode()
    # with them: "score" and nothing else
    scored = write_panoptic(pans, images, CATS, str(tmp_path / 'scored'), confs=confs, write_conf=True)
    files2 = _tree(str(tmp_path / 'scored'))
    assert sorted(set(files2) - set(files)) == ['conf/im0.png', 'conf/im1.png']
    assert all(files2[k] == files[k] for k in files if k != 'pred.json')
    with open(str(tmp_path / 'scored' / 'pred.json')) as f:
        assert json.load(f)['annotations'] == scored
    from PIL import Image
    for i, ((p, c), ann, ann0) in enumerate(zip(maps, scored, plain)):
        assert np.array_equal(np.array(Image.open(str(tmp_path / 'scored' / 'conf' / ('im%d.png' % i)))), c)
        exp = ref.segment_scores(p, c)
        assert segment_scores(p, c) == exp and list(segment_scores(p, c)) == sorted(exp)
        assert [{k: v for k, v in s.items() if k != 'score'} for s in ann['segments_info']] == ann0['segments_info']
        assert [s['score'] for s in ann['segments_info']] == [exp[k][2] for k in sorted(exp)]
    # the filter through the dataset layer == the restatement
    for T in (0.0, 0.5):
        got = filter_by_score(pans, confs, T)
        for (p, c), g in zip(maps, got):
            assert np.array_equal(g.cpu().numpy(), ref.score_filter(p, c, T))
    with pytest.raises(ValueError):
        write_panoptic(pans, images, CATS, str(tmp_path / 'bad'), confs=confs[:1])


def test_old_results_without_planes_are_refused(saved_config):
    from upsnet_amd.evaluate import panoptic_confs
    results = {'all_panos': [None]}
    assert panoptic_confs(results, False, [0]) is None                      # the option is off
    saved_config.test.pan_min_score = 0.5
    with pytest.raises(ValueError, match="all_pano_confs"):
        panoptic_confs(results, False, [0])
    assert panoptic_confs(results, True, [0]) is None                       # the combined merge has no planes
    results['all_pano_confs'] = ['a', 'b']
    assert panoptic_confs(results, False, [1, 0]) == ['b', 'a']


# ------------------------------------------------------------------------------------------------------- end to end on the network
def test_evaluate_end_to_end(tmp_path, saved_config):
    """evaluate.main on the generated COCO-layout dataset: without the option the files are what they were and the pickle holds no
    planes (using it with the option raises); with --pan_confidence the pickle gains 'all_pano_confs', pred.json gains "score" and
    nothing else, the planes are written; --eval_only --pan_min_score filters the same maps the restatement filters."""
    import pickle
    from PIL import Image
    from test_dataset_run_cpu import make_dataset, write_cfg
    from test_dataset_run_gpu import CASES, _direct_chain, _write_gt
    from upsnet_amd.config.config import config, update_config
    from upsnet_amd.dataset import coco
    from upsnet_amd.evaluate import main
    from upsnet_amd.synthetic import build_model
    image_set, sizes = CASES['coco']
    root = str(tmp_path / 'coco')
    make_dataset(root, 'coco', sizes, seed=11)
    cfg = write_cfg(tmp_path, 'coco', root, image_set)
    update_config(cfg)
    ds = coco(image_sets=[image_set], phase='test')
    model = build_model(device='cuda')
    model.use_graph = False
    chains = [_direct_chain(model, e['image'], ds.num_classes) for e in ds.roidb]
    order = [2, 0, 3, 1]
    _write_gt(ds, chains, order, [e['id'] for e in ds.roidb])
    del model
    torch.cuda.empty_cache()
    res = main(['--cfg', cfg, '--synthetic_weights', '--write_panoptic'])
    out = os.path.join(os.path.dirname(res['results_file']), 'pans_unified')
    plain = _tree(out)
    with open(res['results_file'], 'rb') as f:
        assert 'all_pano_confs' not in pickle.load(f)
    with pytest.raises(ValueError, match="all_pano_confs"):
        main(['--cfg', cfg, '--eval_only', '--pan_confidence', '--write_panoptic'])
    config.test.pan_confidence = False
    on = main(['--cfg', cfg, '--synthetic_weights', '--pan_confidence', '--write_panoptic', '--write_pan_confidence'])
    assert on['metrics']['panoptic'] == res['metrics']['panoptic']
    scored = _tree(out)
    assert sorted(set(scored) - set(plain)) == sorted('conf/' + n[4:] for n in plain if n.startswith('pan/'))
    assert all(scored[k] == plain[k] for k in plain if k != 'pred.json')
    with open(on['results_file'], 'rb') as f:
        results = pickle.load(f)
    anns = json.loads(scored['pred.json'])['annotations']
    anns0 = json.loads(plain['pred.json'])['annotations']
    assert [[{k: v for k, v in s.items() if k != 'score'} for s in a['segments_info']] for a in anns] == [a['segments_info'] for a in anns0]
    maps = []
    for a, k in zip(anns, order):
        conf = results['all_pano_confs'][k]
        pan = np.array(Image.open(os.path.join(out, 'pan_2ch', a['file_name'])))
        assert conf.dtype == np.uint8 and conf.shape == pan.shape[:2] == results['all_panos'][k].shape
        assert np.array_equal(np.array(Image.open(os.path.join(out, 'conf', a['file_name']))), conf)
        exp = ref.segment_scores(pan, conf)
        assert [s['score'] for s in a['segments_info']] == [exp[key][2] for key in sorted(exp)]
        maps.append((pan, conf, exp))
    assert any(len(a['segments_info']) >= 3 for a in anns)
    # a threshold between the scores of the run: some segments go, some stay; the files are the restatement's
    every = sorted(s[2] for _, _, exp in maps for s in exp.values())
    T = float(np.float32((every[len(every) // 2 - 1] + every[len(every) // 2]) / 2)) if len(every) > 1 else 0.5
    config.test.pan_confidence = False
    main(['--cfg', cfg, '--eval_only', '--pan_min_score', repr(T), '--write_panoptic'])
    with open(os.path.join(out, 'pred.json')) as f:
        kept = json.load(f)['annotations']
    for a, (pan, conf, exp) in zip(kept, maps):
        want = ref.score_filter(pan, conf, T)
        assert np.array_equal(np.array(Image.open(os.path.join(out, 'pan_2ch', a['file_name']))), want)
        exp2 = ref.segment_scores(want, conf)
        assert [s['score'] for s in a['segments_info']] == [exp2[key][2] for key in sorted(exp2)] and all(s['score'] >= T for s in a['segments_info'])
    assert sum(len(a['segments_info']) for a in kept) < sum(len(a['segments_info']) for a in anns)
