"""COCO, test phase: the reference's file layout (upsnet/dataset/coco.py:47-77) under config.dataset.dataset_path."""
import os

from ..config.config import config
from .json_dataset import TestDataset


class coco(TestDataset):

    prefix = 'coco_'

    def __init__(self, image_sets, flip=False, proposal_files=None, phase='test', result_path=''):
        root = config.dataset.dataset_path
        self.image_dirs = {
            'train2014': os.path.join(root, 'coco_train2014'),
            'val2014': os.path.join(root, 'coco_val2014'),
            'minival2014': os.path.join(root, 'coco_val2014'),
            'valminusminival2014': os.path.join(root, 'coco_val2014'),
            'test2015': os.path.join(root, 'coco_test2015'),
            'test-dev2015': os.path.join(root, 'coco_test2015'),
            'train2017': os.path.join(root, 'images', 'train2017'),
            'val2017': os.path.join(root, 'images', 'val2017'),
            'test-dev2017': os.path.join(root, 'images', 'test2017'),
        }
        self.anno_files = {
            'train2014': 'instances_train2014.json',
            'val2014': 'instances_val2014.json',
            'minival2014': 'instances_minival2014.json',
            'valminusminival2014': 'instances_valminusminival2014.json',
            'test2015': 'image_info_test2015.json',
            'test-dev2015': 'image_info_test-dev2015.json',
            'train2017': 'instances_train2017.json',
            'val2017': 'instances_val2017.json',
            'test-dev2017': 'image_info_test-dev2017.json',
        }
        super(coco, self).__init__(image_sets, flip, proposal_files, phase, result_path)
        self.num_classes = self.dataset.num_classes

    def set_panoptic_files(self, image_set):
        root = os.path.join(config.dataset.dataset_path, 'annotations')
        if image_set == 'test-dev2017':
            self.panoptic_json_file = os.path.join(root, 'image_info_test-dev2017.json')
            self.panoptic_gt_folder = None
        else:
            self.panoptic_json_file = os.path.join(root, 'panoptic_val2017_stff.json')
            self.panoptic_gt_folder = os.path.join(root, 'panoptic_val2017')

    def seg_gt_path(self, entry):
        """coco.py:230: the image path with 'images' -> 'annotations', 'train2017' / 'val2017' -> the semantic train-id folders
        and 'jpg' -> 'png'."""
        return (entry['image'].replace('images', 'annotations').replace('train2017', 'panoptic_train2017_semantic_trainid_stff')
                .replace('val2017', 'panoptic_val2017_semantic_trainid_stff').replace('jpg', 'png'))
