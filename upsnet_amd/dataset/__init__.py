from .cityscapes import Cityscapes
from .coco import coco
from .boundary import boundary_dilation, mask_to_boundary
from .pan_track import PanopticTracker, track_sequence
from .video_pq import VideoPanopticEvaluator
from .mots import MOTSEvaluator
from .pan_components import clean_panoptic
