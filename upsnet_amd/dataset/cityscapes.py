"""Cityscapes, test phase: the reference's file layout (upsnet/dataset/cityscapes.py:45-62) under config.dataset.dataset_path.

One deliberate deviation: the reference reads the panoptic GT PNGs from 'data/cityscapes/panoptic' relative to the working
directory; here they are read from <dataset_path>/panoptic. Likewise the instance-level evaluation reads the gtFine instanceIds
maps from <dataset_path>/gtFine, where the reference points the devkit's CITYSCAPES_DATASET at 'data/cityscapes'."""
import logging
import os

import numpy as np

from ..config.config import config
from .json_dataset import TestDataset


logger = logging.getLogger(__name__)


class Cityscapes(TestDataset):

    prefix = 'cityscapes_'

    def __init__(self, image_sets, flip=False, proposal_files=None, phase='test', result_path=''):
        root = config.dataset.dataset_path
        self.image_dirs = {k: os.path.join(root, 'images') for k in ('train', 'val', 'test', 'train_extra', 'debug')}
        self.anno_files = {
            'train': 'instancesonly_gtFine_train.json',
            'val': 'instancesonly_gtFine_val.json',
            'test': 'image_info_test.json',
            'train_extra': 'instancesonly_gtCoarse_train_extra.json',
            'debug': 'instancesonly_gtFine_debug.json',
        }
        super(Cityscapes, self).__init__(image_sets, flip, proposal_files, phase, result_path)
        self.num_classes = 9

    def set_panoptic_files(self, image_set):
        self.panoptic_json_file = os.path.join(config.dataset.dataset_path, 'annotations', 'cityscapes_fine_val.json')
        self.panoptic_gt_folder = os.path.join(config.dataset.dataset_path, 'panoptic')

    def seg_gt_path(self, entry):
        """cityscapes.py:451: the image path with 'images' -> 'labels' and 'leftImg8bit.png' -> 'gtFine_labelTrainIds.png'."""
        return entry['image'].replace('images', 'labels').replace('leftImg8bit.png', 'gtFine_labelTrainIds.png')

    def instance_gt_path(self, entry):
        """<dataset_path>/gtFine/<split>/<city>/<base>_gtFine_instanceIds.png for the image <base>_leftImg8bit.png, city = the part of
        base before the first underscore: the layout the devkit globs under CITYSCAPES_DATASET."""
        name = os.path.basename(entry['image'])
        if not name.endswith('_leftImg8bit.png'):
            raise ValueError('%s: not a Cityscapes image name (<base>_leftImg8bit.png)' % entry['image'])
        base = name[:-len('_leftImg8bit.png')]
        return os.path.join(config.dataset.dataset_path, 'gtFine', self.image_sets[0], base.split('_')[0],
                            base + '_gtFine_instanceIds.png')

    def check_instance_files(self):
        """FileNotFoundError naming the first missing instance-id map (the files --eval_instances adds to a run's upfront checks)."""
        for e in self.roidb:
            p = self.instance_gt_path(e)
            if not os.path.isfile(p):
                raise FileNotFoundError('%s: file not found: %s' % (self.name, p))

    def load_instance_gt(self, entry):
        """The uint16 [H, W] instance-id map of one image (PIL mode I;16); an unreadable or wrongly sized map raises, naming the file."""
        from PIL import Image
        path = self.instance_gt_path(entry)
        try:
            with Image.open(path) as im:
                if im.mode not in ('I;16', 'I;16L', 'I;16B', 'I', 'L'):
                    raise ValueError('mode %s, not a 16-bit id map' % im.mode)
                gt = np.asarray(im)
        except (OSError, ValueError) as e:
            raise ValueError('%s: cannot read the instance-id map %s: %s' % (self.name, path, e))
        if gt.ndim != 2 or gt.min() < 0 or gt.max() > 65535:
            raise ValueError('%s: %s is not a 16-bit id map' % (self.name, path))
        if gt.shape != (entry['height'], entry['width']):
            raise ValueError('%s: instance-id map %s is %d x %d, its image %d x %d' % (self.name, path, gt.shape[0], gt.shape[1],
                                                                                     entry['height'], entry['width']))
        return np.ascontiguousarray(gt.astype(np.uint16))

    def evaluate_instances(self, all_boxes, all_segms, output_dir):
        """Cityscapes instance-level AP (the devkit's evalInstanceLevelSemanticLabeling, which the reference's
        Cityscapes.evaluate_masks calls, cityscapes.py:347-397) of all_segms[class][image] (im_post's RLE dicts) scored by
        all_boxes[class][image][:, 4], against the gtFine instanceIds maps, on the device (dataset/cityscapes_eval.py). Logs the
        devkit's table, writes it to instance_results.txt and returns {'AP', 'AP50', 'per_class', 'aps'}. Unlike the reference no
        mask PNGs or pred.txt files are written: they are the devkit's input format, not a result."""
        from .cityscapes_eval import InstanceEvaluator, results_lines
        n_cls = len(all_boxes)
        for c in range(1, n_cls):
            if len(all_boxes[c]) != len(self.roidb) or len(all_segms[c]) != len(self.roidb):
                raise ValueError('class %d: results for %d images, the image list has %d' % (c, len(all_boxes[c]), len(self.roidb)))
        ev = InstanceEvaluator()
        for i, entry in enumerate(self.roidb):
            ev.add_rle(self.load_instance_gt(entry), [[]] + [all_boxes[c][i] for c in range(1, n_cls)],
                       [[]] + [all_segms[c][i] for c in range(1, n_cls)])
        res = ev.summary()
        lines = results_lines(res)
        for line in lines:
            logger.info(line)
        os.makedirs(output_dir, exist_ok=True)
        with open(os.path.join(output_dir, 'instance_results.txt'), 'w') as f:
            for line in lines:
                f.write(line + '\n')
        return res
