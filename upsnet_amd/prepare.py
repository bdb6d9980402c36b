"""python -m upsnet_amd.prepare: the evaluation ground truth from the raw dataset downloads (dataset/prepare.py)."""
import logging
import sys

from .dataset.prepare import main, prepare_cityscapes, prepare_coco  # noqa: F401

if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO, format='%(message)s')
    try:
        main()
    except (FileExistsError, FileNotFoundError, ValueError) as e:
        sys.exit('upsnet_amd.prepare: %s' % e)
