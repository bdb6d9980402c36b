"""Test-phase datasets over a COCO-format instances JSON: the roidb of the reference's JsonDataset.get_roidb (upsnet/dataset/
json_dataset.py:60-145) without training fields, image decoding equivalent to cv2.imread(IMREAD_COLOR), the upfront file checks
of a run, evaluate_ssegs over the GT label PNGs, and the pairing of predictions with the panoptic JSON's annotations.

Only phase='test' without flipping or proposal files is implemented: anything else raises NotImplementedError."""
import json
import logging
import os

import numpy as np
import torch

from .. import ops
from ..config.config import config
from .base_dataset import BaseDataset
from .restore import pil_nearest_tables

logger = logging.getLogger(__name__)


def imread_bgr(path):
    """cv2.imread(path, IMREAD_COLOR) with PIL: EXIF orientation applied, grayscale / palette / CMYK / alpha images converted to
    three colour channels, BGR channel order; uint8 [H,W,3]. A missing or unreadable file raises."""
    from PIL import Image, ImageOps
    with Image.open(path) as im:
        im = ImageOps.exif_transpose(im)
        if im.mode != 'RGB':
            im = im.convert('RGB')
        rgb = np.asarray(im)
    return np.ascontiguousarray(rgb[:, :, ::-1])


class JsonDataset(object):
    """The image list of a COCO-format JSON: image ids ascending (json_dataset.py:103-104), entry['image'] = image_dir joined with
    the file name (:137-139), the category table in JSON order."""

    def __init__(self, name, image_dir, anno_file):
        self.name = name
        self.image_directory = image_dir
        self.anno_file = anno_file
        if not os.path.isfile(anno_file):
            raise FileNotFoundError('annotation file not found: %s' % anno_file)
        with open(anno_file, 'r') as f:
            js = json.load(f)
        self.category_ids = [int(c['id']) for c in js.get('categories', [])]
        self.classes = ['__background__'] + [c['name'] for c in js.get('categories', [])]
        self.num_classes = len(self.classes)
        self.images = {int(im['id']): im for im in js['images']}

    def get_roidb(self):
        roidb = []
        for image_id in sorted(self.images):
            im = self.images[image_id]
            roidb.append({'id': image_id, 'file_name': im['file_name'], 'height': int(im['height']), 'width': int(im['width']),
                          'image': os.path.join(self.image_directory, im['file_name']), 'flipped': False})
        return roidb


def panoptic_pairing(roidb_ids, ann_image_ids):
    """For each annotation of the panoptic JSON (in its order), the roidb position of its prediction. By image id when the
    annotations' ids are a subset of the roidb's; otherwise by position (the reference's own pairing) if the counts match, which is
    logged; otherwise ValueError."""
    pos = {i: k for k, i in enumerate(roidb_ids)}
    if all(i in pos for i in ann_image_ids):
        return [pos[i] for i in ann_image_ids]
    if len(ann_image_ids) == len(roidb_ids):
        logger.info('panoptic annotations name image ids outside the image list: pairing %d predictions by position, as the '
                    'reference does', len(roidb_ids))
        return list(range(len(roidb_ids)))
    raise ValueError('cannot pair %d predictions with %d panoptic annotations: their image ids are not among the image list'
                     % (len(roidb_ids), len(ann_image_ids)))


class TestDataset(BaseDataset):
    """Common part of Cityscapes / coco. Subclasses set image_dirs, anno_files and panoptic_json_file / panoptic_gt_folder and
    define seg_gt_path(entry)."""

    prefix = ''
    image_dirs = {}
    anno_files = {}

    def __init__(self, image_sets, flip=False, proposal_files=None, phase='test', result_path=''):
        super(TestDataset, self).__init__()
        if phase != 'test':
            raise NotImplementedError("%s: phase %r -- only phase='test' is implemented" % (type(self).__name__, phase))
        if flip:
            raise NotImplementedError('%s: flipped inputs are not implemented' % type(self).__name__)
        if proposal_files is not None and any(p is not None for p in proposal_files):
            raise NotImplementedError('%s: proposal files are not implemented' % type(self).__name__)
        if isinstance(image_sets, str):
            image_sets = image_sets.split('+')
        if len(image_sets) != 1:
            raise NotImplementedError('%s: one image set per run, got %s' % (type(self).__name__, image_sets))
        self.image_sets = image_sets
        self.flip, self.phase, self.result_path = False, phase, result_path
        image_set = image_sets[0]
        if image_set not in self.anno_files:
            raise ValueError('%s: unknown image set %r (known: %s)' % (type(self).__name__, image_set, sorted(self.anno_files)))
        self.set_panoptic_files(image_set)
        self.dataset = JsonDataset(self.prefix + image_set, image_dir=self.image_dirs[image_set],
                                   anno_file=os.path.join(config.dataset.dataset_path, 'annotations', self.anno_files[image_set]))
        self.name = self.dataset.name
        self.instances_json_file = self.dataset.anno_file
        self.roidb = self.dataset.get_roidb()
        # test sets without annotations (image_info_test*.json): inference and the results pickle only
        self.has_gt = not os.path.basename(self.instances_json_file).startswith('image_info')

    def __len__(self):
        return len(self.roidb)

    def set_panoptic_files(self, image_set):
        raise NotImplementedError

    def seg_gt_path(self, entry):
        raise NotImplementedError

    def load_image(self, index):
        return imread_bgr(self.roidb[index]['image'])

    def required_files(self, images=True):
        """Every file a run reads, in the order they are checked: the images, then the GT of the configured heads."""
        files = [e['image'] for e in self.roidb] if images else []
        if not self.has_gt:
            return files
        if config.network.has_fcn_head:
            files += [self.seg_gt_path(e) for e in self.roidb]
        if config.network.has_panoptic_head:
            files.append(self.panoptic_json_file)
            if os.path.isfile(self.panoptic_json_file):
                with open(self.panoptic_json_file, 'r') as f:
                    gt_json = json.load(f)
                files += [os.path.join(self.panoptic_gt_folder, item['file_name']) for item in gt_json['images']]
        return files

    def check_files(self, images=True):
        """FileNotFoundError naming the first missing file of required_files()."""
        for p in self.required_files(images):
            if not os.path.isfile(p):
                raise FileNotFoundError('%s: file not found: %s' % (self.name, p))

    def panoptic_order(self):
        """panoptic_pairing of this image list with the panoptic JSON's annotations."""
        with open(self.panoptic_json_file, 'r') as f:
            anns = json.load(f)['annotations']
        return panoptic_pairing([e['id'] for e in self.roidb], [a['image_id'] for a in anns])

    def evaluate_ssegs(self, pred_segmentations, res_file_folder):
        """mIoU of the uint8 predictions (one per roidb entry, at original image resolution) against the GT label PNGs
        (seg_gt_path); a prediction whose shape differs from its GT is resized with PIL's NEAREST rule on the device first. Pixels
        with GT 255 are ignored; the confusion matrix is counted on the device (evaluate_ssegs_arrays). Unlike the reference no
        prediction PNGs are written to res_file_folder. Returns {'meanIU', 'IU_array', 'confusion_matrix'} and logs them."""
        from PIL import Image
        if len(pred_segmentations) != len(self.roidb):
            raise ValueError('%d semantic predictions for %d images' % (len(pred_segmentations), len(self.roidb)))
        dev = torch.device('cuda', torch.cuda.current_device())
        gts, preds = [], []
        for entry, pred in zip(self.roidb, pred_segmentations):
            gt = np.array(Image.open(self.seg_gt_path(entry)))
            pred = torch.as_tensor(np.asarray(pred)).to(dev)
            pred = pred.reshape(pred.shape[-2], pred.shape[-1])
            if tuple(pred.shape) != gt.shape[:2]:
                y_ofs, x_ofs = pil_nearest_tables(tuple(pred.shape), gt.shape[:2])
                pred, _ = ops.restore_label_maps(pred.to(torch.int64), None, y_ofs, x_ofs)
            gts.append(gt)
            preds.append(pred)
        res = self.evaluate_ssegs_arrays(gts, preds, config.dataset.num_seg_classes)
        logger.info('evaluate segmentation:')
        logger.info('IU_array:')
        for v in res['IU_array']:
            logger.info('%.5f' % v)
        logger.info('meanIU:%.5f' % res['meanIU'])
        return res
