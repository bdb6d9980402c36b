#!/usr/bin/env python
"""Golden vectors for proposal recall, made by the REFERENCE's own BaseDataset.evaluate_box_proposals
(upsnet/dataset/base_dataset.py:723-805), imported from the reference checkout with the in-process shims of make_golden_blob.py.

Those shims stand in a zero matrix for the Cython upsnet.bbox.bbox. Here the reference's own bbox.pyx is cythonised and compiled
with gcc into a temporary directory outside the repository (as oracle/build_ref_cpu_nms.py builds cpu_nms.pyx), imported, and bound
to upsnet.bbox.bbox_transform.bbox_overlaps_cython (bound at import). Nothing compiled is kept.

The scenes cover crowd GT, proposal rows interleaved with GT rows, GT areas exactly on 32^2, 96^2, 128^2, 256^2 and 512^2, an image
with no proposals and one with no valid GT, P < G, duplicated proposals, identical GT boxes and exactly equal IoUs of different pairs
(tie order), proposals that overlap nothing, limit None / 0 / below P, all 8 areas (one with num_pos == 0) and default and custom
thresholds.

Run in the build container:  python tests/golden/make_golden_proposals.py   (writes tests/golden/proposal_recall.npz)
"""
import importlib.util
import json
import os
import shutil
import subprocess
import sys
import sysconfig
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_blob as mgb  # noqa: E402  (shims, the reference checkout on sys.path, the reference's BaseDataset)
import proposal_recall_ref as prr  # noqa: E402  (scene helpers only)

BaseDataset = mgb.BaseDataset
AREAS = list(prr.AREAS)
THRESHOLDS = {'default': None, 'custom': np.array([0.1, 0.5, 0.55, 0.7, 0.9, 1.0])}


def build_bbox_module(tmp):
    src = os.path.join(mgb.mg.REF, 'upsnet', 'bbox', 'bbox.pyx')
    pyx = os.path.join(tmp, 'upsnet_ref_bbox.pyx')
    shutil.copy(src, pyx)
    c = os.path.join(tmp, 'upsnet_ref_bbox.c')
    subprocess.check_call([sys.executable, '-m', 'cython', '-2', pyx, '-o', c], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    so = os.path.join(tmp, 'upsnet_ref_bbox' + sysconfig.get_config_var('EXT_SUFFIX'))
    subprocess.check_call(['gcc', '-O2', '-fPIC', '-shared', '-ffp-contract=off', '-fno-fast-math', '-w',
                           '-I', sysconfig.get_paths()['include'], '-I', np.get_include(), c, '-o', so])
    spec = importlib.util.spec_from_file_location('upsnet_ref_bbox', so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scenes():
    rng = np.random.default_rng(20261016)
    imgs = []

    def add(props, gt, cls, crowd, areas, interleave=True):
        imgs.append(prr.roidb_entry(np.asarray(props, np.float32).reshape(-1, 4), np.asarray(gt, np.float32).reshape(-1, 4),
                                    np.asarray(cls, np.int32), np.asarray(crowd, bool), np.asarray(areas, np.float32),
                                    rng if interleave else None))
    # 0: crowd GT, interleaved rows
    p, g, c, cr, a = prr.random_scene(rng, 60, 12, crowd_frac=0.3)
    add(p, g, c, cr, a)
    # 1: GT areas exactly on the range edges (and one either side)
    edges = [32 ** 2, 96 ** 2, 128 ** 2, 256 ** 2, 512 ** 2]
    areas = [e + d for e in edges for d in (-1, 0, 1)]
    gt = [[10 * i, 5 * i, 10 * i + 60, 5 * i + 40] for i in range(len(areas))]
    p, _, _, _, _ = prr.random_scene(rng, 40, 3)
    props = np.concatenate([np.asarray(gt, np.float32) + np.float32(2), p])
    add(props, gt, np.ones(len(gt)), np.zeros(len(gt)), areas)
    # 2: no proposals
    p, g, c, cr, a = prr.random_scene(rng, 0, 5, crowd_frac=0.0)
    add(p, g, c, cr, a)
    # 3: no valid GT (all crowd)
    p, g, c, cr, a = prr.random_scene(rng, 20, 4)
    add(p, g, c, np.ones(4), a)
    # 4: P < G
    p, g, c, cr, a = prr.random_scene(rng, 3, 10, crowd_frac=0.0)
    add(p, g, c, cr, a)
    # 5: identical GT boxes, duplicated proposals, equal IoUs of different pairs (mirror-image shifts)
    gt = [[100, 100, 139, 139]] * 3 + [[300, 300, 319, 339], [200, 100, 239, 139]]
    props = [[98, 100, 137, 139], [102, 100, 141, 139], [98, 100, 137, 139], [100, 98, 139, 137], [100, 102, 139, 141],
             [298, 300, 317, 339], [302, 300, 321, 339], [198, 100, 237, 139], [202, 100, 241, 139], [100, 100, 139, 139],
             [100, 100, 139, 139]]
    add(props, gt, [1, 2, 3, 4, 5], [0, 0, 0, 0, 0], [1600, 1600, 1600, 800, 1600])
    # 6: proposals that overlap nothing
    add([[900, 700, 950, 760], [0, 700, 10, 790], [1000, 0, 1020, 20]], [[100, 100, 200, 150], [300, 50, 330, 90]], [1, 1], [0, 0],
        [5000, 1200])
    # 7: a larger random image with integer coordinates (ties) and duplicates
    p, g, c, cr, a = prr.random_scene(rng, 300, 40, dup_frac=0.1)
    add(p, g, c, cr, a)
    # 8: large GT (area over 512^2 is absent from images 0-7 except image 1's edge set)
    p, g, c, cr, a = prr.random_scene(rng, 50, 6, crowd_frac=0.0)
    add(p, g, c, cr, a)
    return imgs


def main():
    imgs = scenes()
    calls = []
    everything = list(range(len(imgs)))
    for area in AREAS:
        for limit in (None, 0, 5, 100):
            calls.append((everything, area, limit, 'default'))
        calls.append((everything, area, 20, 'custom'))
    # num_pos == 0: no GT of 512^2 or more outside image 1
    calls.append(([i for i in everything if i != 1], '512-inf', None, 'default'))
    calls.append(([2, 3], 'all', None, 'custom'))
    tmp = tempfile.mkdtemp(prefix='upsnet_ref_bbox_')
    try:
        bbox_mod = build_bbox_module(tmp)
        bt = sys.modules['upsnet.bbox.bbox_transform']
        assert bt.__file__.startswith(mgb.mg.REF + os.sep)
        bt.bbox_overlaps_cython = bbox_mod.bbox_overlaps
        ds = BaseDataset.__new__(BaseDataset)
        out = {}
        for k, (inds, area, limit, thr) in enumerate(calls):
            res = BaseDataset.evaluate_box_proposals(ds, [imgs[i] for i in inds], thresholds=THRESHOLDS[thr], area=area, limit=limit)
            for f in ('recalls', 'thresholds', 'gt_overlaps'):
                out['call%d_%s' % (k, f)] = np.asarray(res[f])
            out['call%d_ar' % k] = np.asarray(res['ar'], np.float64)
            out['call%d_num_pos' % k] = np.asarray(res['num_pos'], np.int64)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for i, e in enumerate(imgs):
        for f in ('boxes', 'gt_classes', 'is_crowd', 'seg_areas'):
            out['img%d_%s' % (i, f)] = e[f]
    out['spec'] = np.asarray(json.dumps({'num_images': len(imgs), 'calls': calls,
                                         'thresholds': {k: (None if v is None else v.tolist()) for k, v in THRESHOLDS.items()}}))
    path = os.path.join(HERE, 'proposal_recall.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', len(calls), 'calls')


if __name__ == '__main__':
    main()
