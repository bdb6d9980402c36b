#!/usr/bin/env python
"""Golden data for the COCO stuff-first category remap, made by the REFERENCE's own init_coco.py: the script is run unchanged, as a
child process, in a temporary directory that holds a synthetic 133-category table (lib/dataset_devkit/panopticapi/
panoptic_coco_categories.json) and synthetic panoptic_{train,val}2017.json files. Only data is stored: the synthetic input and,
from the files the script wrote, the category ids per segment, the image order, the file names and the category table.

Run in the build container:  python tests/golden/make_golden_coco_stff.py [reference checkout]   (writes tests/golden/coco_stff.json)
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def synthetic_categories():
    """133 categories in the download's order: 80 things with COCO-like gapped ids, then 53 stuff classes."""
    thing_ids = [i for i in range(1, 91) if i not in (12, 26, 29, 30, 45, 66, 68, 69, 71, 83)]
    stuff_ids = list(range(92, 92 + 2 * 53, 2))
    cats = [{'supercategory': 'sup%d' % (i % 7), 'isthing': 1, 'id': i, 'name': 'thing%d' % i,
             'color': [(37 * i) % 256, (91 * i + 5) % 256, (53 * i + 11) % 256]} for i in thing_ids]
    cats += [{'supercategory': 'ssup%d' % (i % 5), 'isthing': 0, 'id': i, 'name': 'stuff%d' % i,
              'color': [(41 * i) % 256, (17 * i + 3) % 256, (29 * i + 7) % 256]} for i in stuff_ids]
    assert len(cats) == 133
    return cats


def synthetic_panoptic(cats, image_ids):
    """Every category occurs; images in the given (unsorted) order, annotations in another."""
    images = [{'id': i, 'file_name': '%012d.jpg' % i, 'height': 8, 'width': 8} for i in image_ids]
    anns = []
    for k, i in enumerate(reversed(image_ids)):
        segs = [{'id': 1000 * (k + 1) + j, 'category_id': c['id'], 'iscrowd': int(j % 9 == 0), 'area': 1 + j, 'bbox': [0, 0, 1, 1]}
                for j, c in enumerate(cats) if j % len(image_ids) == k]
        anns.append({'image_id': i, 'file_name': '%012d.png' % i, 'segments_info': segs})
    return {'info': {'description': 'synthetic'}, 'images': images, 'annotations': anns, 'categories': cats}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    cats = synthetic_categories()
    inputs = {'train': synthetic_panoptic(cats, [9, 2, 7]), 'val': synthetic_panoptic(cats, [139, 5, 77, 42])}
    out = {'inputs': inputs, 'expected': {}}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'lib', 'dataset_devkit', 'panopticapi'))
        os.makedirs(os.path.join(tmp, 'data', 'coco', 'annotations'))
        with open(os.path.join(tmp, 'lib', 'dataset_devkit', 'panopticapi', 'panoptic_coco_categories.json'), 'w') as f:
            json.dump(cats, f)
        for s, js in inputs.items():
            with open(os.path.join(tmp, 'data', 'coco', 'annotations', 'panoptic_%s2017.json' % s), 'w') as f:
                json.dump(js, f)
        subprocess.check_call([sys.executable, os.path.join(ref, 'init_coco.py')], cwd=tmp)
        ann = os.path.join(tmp, 'data', 'coco', 'annotations')
        with open(os.path.join(ann, 'panoptic_coco_categories_stff.json')) as f:
            out['expected']['categories'] = json.load(f)
        for s in inputs:
            with open(os.path.join(ann, 'panoptic_%s2017_stff.json' % s)) as f:
                js = json.load(f)
            out['expected'][s] = {
                'image_ids': [im['id'] for im in js['images']],
                'file_names': [im['file_name'] for im in js['images']],
                'annotation_image_ids': [a['image_id'] for a in js['annotations']],
                'segment_categories': [[[seg['id'], seg['category_id']] for seg in a['segments_info']] for a in js['annotations']],
                'categories_equal_table': js['categories'] == out['expected']['categories'],
            }
    path = os.path.join(HERE, 'coco_stff.json')
    with open(path, 'w') as f:
        json.dump(out, f, sort_keys=True)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
