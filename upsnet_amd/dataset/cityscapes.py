"""Cityscapes, test phase: the reference's file layout (upsnet/dataset/cityscapes.py:45-62) under config.dataset.dataset_path.

One deliberate deviation: the reference reads the panoptic GT PNGs from 'data/cityscapes/panoptic' relative to the working
directory; here they are read from <dataset_path>/panoptic."""
import os

from ..config.config import config
from .json_dataset import TestDataset


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
