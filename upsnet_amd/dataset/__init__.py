from .cityscapes import Cityscapes
from .coco import coco
