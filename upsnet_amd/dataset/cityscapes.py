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

    # ---------------------------------------------------------------------------------------------- pixel-level IoU / iIoU
    def label_gt_path(self, entry):
        """<dataset_path>/gtFine/<split>/<city>/<base>_gtFine_labelIds.png, next to instance_gt_path."""
        return self.instance_gt_path(entry)[:-len('instanceIds.png')] + 'labelIds.png'

    def check_pixel_files(self):
        """FileNotFoundError naming the first missing label-id or instance-id map (the files --eval_pixels adds to the upfront checks)."""
        for e in self.roidb:
            for p in (self.label_gt_path(e), self.instance_gt_path(e)):
                if not os.path.isfile(p):
                    raise FileNotFoundError('%s: file not found: %s' % (self.name, p))

    def load_label_gt(self, entry):
        """The uint8 [H, W] label-id map of one image; an unreadable or wrongly sized map raises, naming the file."""
        from PIL import Image
        path = self.label_gt_path(entry)
        try:
            with Image.open(path) as im:
                if im.mode not in ('L', 'P'):
                    raise ValueError('mode %s, not an 8-bit label map' % im.mode)
                gt = np.asarray(im)
        except (OSError, ValueError) as e:
            raise ValueError('%s: cannot read the label-id map %s: %s' % (self.name, path, e))
        if gt.ndim != 2 or gt.shape != (entry['height'], entry['width']):
            raise ValueError('%s: label-id map %s is %s, its image %d x %d' % (self.name, path, ' x '.join(str(s) for s in gt.shape),
                                                                               entry['height'], entry['width']))
        return np.ascontiguousarray(gt.astype(np.uint8))

    def _report_pixels(self, ev, output_dir):
        from .cityscapes_pixel_eval import results_lines
        res = ev.summary()
        lines = results_lines(res)
        for line in lines:
            logger.info(line)
        if output_dir is not None:
            os.makedirs(output_dir, exist_ok=True)
            with open(os.path.join(output_dir, 'pixel_results.txt'), 'w') as f:
                for line in lines:
                    f.write(line + '\n')
        return res

    def evaluate_pixels(self, pred_segmentations, output_dir):
        """Cityscapes pixel-level IoU / iIoU (the devkit's evalPixelLevelSemanticLabeling) of the semantic predictions as
        evaluate_ssegs takes them (train ids, one per roidb entry; a prediction whose shape differs from its ground truth is resized
        with PIL's NEAREST rule on the device first) against the gtFine labelIds and instanceIds maps, on the device
        (dataset/cityscapes_pixel_eval.py). Logs the devkit-style tables, writes them to pixel_results.txt and returns
        {'IoU_class', 'iIoU_class', 'IoU_category', 'iIoU_category', 'per_class', 'per_category', 'conf', 'wsum'}."""
        import torch
        from .. import ops
        from .cityscapes_pixel_eval import PixelEvaluator
        from .restore import pil_nearest_tables
        if len(pred_segmentations) != len(self.roidb):
            raise ValueError('%d semantic predictions for %d images' % (len(pred_segmentations), len(self.roidb)))
        dev = torch.device('cuda', torch.cuda.current_device())
        ev = PixelEvaluator(dev)
        for entry, pred in zip(self.roidb, pred_segmentations):
            labels, ids = self.load_label_gt(entry), self.load_instance_gt(entry)
            pred = np.asarray(pred)
            if pred.min() < 0 or pred.max() > 255:       # (a uint8 cast would wrap such a value into a valid train id)
                raise ValueError('%s: the prediction of %s holds values outside 0..255' % (self.name, entry['image']))
            pred = torch.as_tensor(pred).to(dev)
            pred = pred.reshape(pred.shape[-2], pred.shape[-1])
            if tuple(pred.shape) != labels.shape:
                y_ofs, x_ofs = pil_nearest_tables(tuple(pred.shape), labels.shape)
                pred, _ = ops.restore_label_maps(pred.to(torch.int64), None, y_ofs, x_ofs)
            ev.add(labels, ids, pred.to(torch.uint8), train_ids=True, name=os.path.basename(entry['image']))
        return self._report_pixels(ev, output_dir)

    def segmentation_result_path(self, entry, res_file_folder):
        """cityscapes.py:507-509: <folder>/<base>.png for the image <base>_leftImg8bit.png."""
        return os.path.join(res_file_folder, os.path.basename(entry['image'])[:-len('_leftImg8bit.png')] + '.png')

    def get_pallete(self):
        """The reference's palette (cityscapes.py:399-442): 256 x 3 bytes, entry t < 19 the colour of train id t, the rest zero."""
        from .cityscapes_pixel_eval import TRAIN_ID_COLOURS
        pallete = np.zeros((256, 3), np.uint8)
        pallete[:len(TRAIN_ID_COLOURS)] = TRAIN_ID_COLOURS
        return pallete.reshape(-1)

    def write_segmentation_result(self, segmentation_results, res_file_folder, label_ids=False):
        """The reference's write_segmentation_result (cityscapes.py:494-514): one palette PNG of train ids per image, named
        <base>.png, with the palette of get_pallete. label_ids=True writes grey 8-bit PNGs of label ids instead, the format the
        benchmark server takes; the train id -> label id look-up runs on the host (the predictions are host arrays already, and a
        256-entry take is a thousandth of the PNG encoding beside it). A value that is no train id raises ValueError."""
        from PIL import Image
        from .cityscapes_pixel_eval import NOT_A_LABEL, lookup_table
        if len(segmentation_results) != len(self.roidb):
            raise ValueError('%d semantic predictions for %d images' % (len(segmentation_results), len(self.roidb)))
        os.makedirs(res_file_folder, exist_ok=True)
        pallete, lut = self.get_pallete(), lookup_table(True)
        for entry, seg in zip(self.roidb, segmentation_results):
            seg = np.squeeze(np.copy(seg))
            if seg.min() < 0 or seg.max() > 255:
                raise ValueError('%s: the prediction of %s holds values outside 0..255' % (self.name, entry['image']))
            seg = np.uint8(seg)
            if label_ids:
                seg = lut[seg]
                if (seg == NOT_A_LABEL).any():
                    raise ValueError('%s: the prediction of %s holds values that are no train id' % (self.name, entry['image']))
                im = Image.fromarray(seg)
            else:
                im = Image.fromarray(seg)
                im.putpalette(pallete)
            im.save(self.segmentation_result_path(entry, res_file_folder))
        logger.info('%d semantic predictions (%s) written to %s', len(self.roidb), 'label ids' if label_ids else 'train ids, palette',
                    os.path.abspath(res_file_folder))

    def evaluate_pixels_files(self, folder, output_dir=None):
        """evaluate_pixels over a written folder: <folder>/<base>.png per image, palette PNGs (mode P) holding train ids or grey PNGs
        (mode L) holding label ids -- write_segmentation_result's output or another tool's submission. A prediction of another size
        than its ground truth is resized with PIL's NEAREST, as the reference does when it reads its files back. A missing file, or
        one of another mode, raises naming it."""
        from PIL import Image
        from .cityscapes_pixel_eval import PixelEvaluator
        ev = PixelEvaluator()
        for entry in self.roidb:
            path = self.segmentation_result_path(entry, folder)
            if not os.path.isfile(path):
                raise FileNotFoundError('%s: no prediction for %s at %s' % (self.name, os.path.basename(entry['image']), path))
            labels, ids = self.load_label_gt(entry), self.load_instance_gt(entry)
            with Image.open(path) as im:
                if im.mode not in ('P', 'L'):
                    raise ValueError('%s: mode %s; a palette PNG (train ids) or a grey 8-bit PNG (label ids) is expected' % (path, im.mode))
                train_ids = im.mode == 'P'
                if (im.size[1], im.size[0]) != labels.shape:
                    im = im.resize((labels.shape[1], labels.shape[0]), Image.NEAREST)
                pred = np.array(im, dtype=np.uint8)
            ev.add(labels, ids, pred, train_ids=train_ids, name=path)
        return self._report_pixels(ev, output_dir)

    # ---------------------------------------------------------------------------------------------- detection visualisations
    def vis_all_mask(self, all_boxes, all_masks, save_path=None):
        """The reference's override (cityscapes.py:236-345): as BaseDataset.vis_all_mask with the eight instance classes by name and
        every mask in its class's colour (train ids 11..18 of the palette); PNGs named <base>.png for the image <base>_leftImg8bit.png
        (the basename minus its last 16 characters)."""
        from . import vis
        from .cityscapes_eval import CLASS_NAMES
        from .cityscapes_pixel_eval import TRAIN_ID_COLOURS
        first_thing = len(TRAIN_ID_COLOURS) - len(CLASS_NAMES)
        return vis.vis_all_mask(self, all_boxes, all_masks, ('__background__',) + tuple(CLASS_NAMES),
                                lambda j, k: TRAIN_ID_COLOURS[first_thing + j - 1],
                                lambda entry: '{}.png'.format(entry['image'].split('/')[-1][:-16]), save_path)

    def evaluate_instances(self, all_boxes, all_segms, output_dir):
        """Cityscapes instance-level AP (the devkit's evalInstanceLevelSemanticLabeling, which the reference's
        Cityscapes.evaluate_masks calls, cityscapes.py:347-397) of all_segms[class][image] (im_post's RLE dicts) scored by
        all_boxes[class][image][:, 4], against the gtFine instanceIds maps, on the device (dataset/cityscapes_eval.py). Logs the
        devkit's table, writes it to instance_results.txt and returns {'AP', 'AP50', 'per_class', 'aps'}. Unlike the reference no
        mask PNGs or pred.txt files are written here: they are the devkit's input format, not a result (write_instance_result writes
        them, evaluate_instances_files scores them)."""
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

    def write_instance_result(self, all_boxes, all_segms, output_dir, one_bit=False):
        """The files of the reference's evaluate_masks (cityscapes.py:368-395), the benchmark server's instance-level format:
        <output_dir>/inst_seg/<basename>pred.txt and one mask PNG per detection under inst_seg/seg_results/<basename>/, 8-bit grey
        0 / 255 or, with one_bit, bit depth 1 (dataset/cityscapes_inst_format.py). Needs no ground truth. Returns the txt paths."""
        from .cityscapes_inst_format import write_instance_predictions
        return write_instance_predictions(self, all_boxes, all_segms, output_dir, one_bit=one_bit)

    def evaluate_instances_files(self, folder, output_dir=None):
        """evaluate_instances over a folder in the benchmark's format (write_instance_result's output or another tool's submission;
        the devkit's file rules are restated in dataset/cityscapes_inst_format.py): the same table logged, written to
        <output_dir>/instance_results.txt when output_dir is given, the same dict returned."""
        from .cityscapes_eval import results_lines
        from .cityscapes_inst_format import score_instance_files
        if not self.has_gt:
            raise ValueError('%s has no ground truth to score against' % self.name)
        self.check_instance_files()
        res = score_instance_files(self, folder).summary()
        lines = results_lines(res)
        for line in lines:
            logger.info(line)
        if output_dir is not None:
            os.makedirs(output_dir, exist_ok=True)
            with open(os.path.join(output_dir, 'instance_results.txt'), 'w') as f:
                for line in lines:
                    f.write(line + '\n')
        return res
