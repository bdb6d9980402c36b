"""Numpy restatement of the Cityscapes devkit's pixel-level evaluation (evalPixelLevelSemanticLabeling, its Python path) on FULL
maps, for the tests of dataset/cityscapes_pixel_eval.py: a confusion matrix filled pixel pair by pixel pair, `np.unique` over the
instance-id map, `np.count_nonzero` over `==` masks, Python-float accumulation in the devkit's order. It shares no code with the
product and imports nothing from it.

An image is (gt_labels uint8 [H, W], gt_ids uint16 [H, W] or None, pred uint8 [H, W] of LABEL ids). `evaluate(images, avg, stats)`
fills `stats` (a dict of counters) with how often each branch of the rules was taken."""
import math

import numpy as np

# id: (name, category, hasInstances, ignoreInEval)
LABELS = {
    0: ('unlabeled', 'void', False, True), 1: ('ego vehicle', 'void', False, True), 2: ('rectification border', 'void', False, True),
    3: ('out of roi', 'void', False, True), 4: ('static', 'void', False, True), 5: ('dynamic', 'void', False, True),
    6: ('ground', 'void', False, True), 7: ('road', 'flat', False, False), 8: ('sidewalk', 'flat', False, False),
    9: ('parking', 'flat', False, True), 10: ('rail track', 'flat', False, True), 11: ('building', 'construction', False, False),
    12: ('wall', 'construction', False, False), 13: ('fence', 'construction', False, False),
    14: ('guard rail', 'construction', False, True), 15: ('bridge', 'construction', False, True),
    16: ('tunnel', 'construction', False, True), 17: ('pole', 'object', False, False), 18: ('polegroup', 'object', False, True),
    19: ('traffic light', 'object', False, False), 20: ('traffic sign', 'object', False, False),
    21: ('vegetation', 'nature', False, False), 22: ('terrain', 'nature', False, False), 23: ('sky', 'sky', False, False),
    24: ('person', 'human', True, False), 25: ('rider', 'human', True, False), 26: ('car', 'vehicle', True, False),
    27: ('truck', 'vehicle', True, False), 28: ('bus', 'vehicle', True, False), 29: ('caravan', 'vehicle', True, True),
    30: ('trailer', 'vehicle', True, True), 31: ('train', 'vehicle', True, False), 32: ('motorcycle', 'vehicle', True, False),
    33: ('bicycle', 'vehicle', True, False),
}
CATEGORY_ORDER = ['void', 'flat', 'construction', 'object', 'nature', 'sky', 'human', 'vehicle']
TRAIN2LABEL = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]
# a table of the tests' own: nothing depends on the product's default being right
AVG = {'person': 3462.4756337644, 'rider': 3930.4788056518, 'car': 12794.0202738185, 'truck': 27855.1264367816, 'bus': 35732.1511111111,
       'train': 67583.7075812274, 'motorcycle': 6298.7200839748, 'bicycle': 4672.3249222261}
OTHER_AVG = {'person': 1000.0, 'rider': 333.3, 'car': 7.0, 'truck': 123456.789, 'bus': 0.1, 'train': 2.0 ** 20, 'motorcycle': 3.0, 'bicycle': 1e6 / 3}
INSTANCE_CLASSES = ['person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle']


def _bump(stats, key, n=1):
    if stats is not None:
        stats[key] = stats.get(key, 0) + n


def category_labels(cat):
    return [l for l in sorted(LABELS) if LABELS[l][1] == cat]


def evaluate_pair(gt_labels, gt_ids, pred, conf, inst_stats, avg, stats=None):
    """evaluatePair: adds one image to conf (int64 [34, 34]) and inst_stats; returns {raw value: (size, tp, category tp)}."""
    assert gt_labels.shape == pred.shape and pred.max() < 34 and gt_labels.max() < 34
    for g in np.unique(gt_labels):
        for p in np.unique(pred):
            conf[int(g), int(p)] += int(np.count_nonzero(np.logical_and(gt_labels == g, pred == p)))
    table = {}
    if gt_ids is None:
        return None
    cat_masks = {}
    for cat in inst_stats['categories']:
        m = np.zeros(pred.shape, bool)
        for l in category_labels(cat):
            if not LABELS[l][3]:
                m = np.logical_or(m, pred == l)
        cat_masks[cat] = m
    for inst_id in np.unique(gt_ids[gt_ids > 1000]):
        inst_id = int(inst_id)
        label_id = int(inst_id / 1000)
        if label_id not in LABELS:
            _bump(stats, 'instance_of_no_label')
            continue
        name, cat, has_inst, ignore = LABELS[label_id]
        if ignore:
            _bump(stats, 'instance_of_ignored_label')
            continue
        if not has_inst:
            _bump(stats, 'instance_value_of_stuff_label')
            continue
        mask = gt_ids == inst_id
        size = int(np.count_nonzero(mask))
        tp = int(np.count_nonzero(pred[mask] == label_id))
        fn = size - tp
        weight = avg[name] / float(size)
        tp_w = float(tp) * weight
        fn_w = float(fn) * weight
        c = inst_stats['classes'][name]
        c['tp'] += tp
        c['fn'] += fn
        c['tpWeighted'] += tp_w
        c['fnWeighted'] += fn_w
        cat_tp = int(np.count_nonzero(np.logical_and(mask, cat_masks[cat])))
        cat_fn = size - cat_tp
        k = inst_stats['categories'][cat]
        k['tp'] += cat_tp
        k['fn'] += cat_fn
        k['tpWeighted'] += float(cat_tp) * weight
        k['fnWeighted'] += float(cat_fn) * weight
        table[inst_id] = (size, tp, cat_tp)
        _bump(stats, 'instances')
        if inst_id % 1000 == 0:
            _bump(stats, 'instance_number_zero')
        if cat_tp > tp:
            _bump(stats, 'category_hit_of_another_class')
        if 0 < tp < size:
            _bump(stats, 'partly_hit_instance')
    return table


def _score(tp, fp, fn):
    denom = tp + fp + fn
    if denom == 0:
        return float('nan')
    return float(tp) / denom


def score_average(score_list):
    valid, total = 0, 0.0
    for key in score_list:
        if not math.isnan(score_list[key]):
            valid += 1
            total += score_list[key]
    if valid == 0:
        return float('nan')
    return total / valid


def evaluate(images, avg=None, stats=None):
    """{'conf', 'inst' (one table per image), 'inst_stats', 'classScores', 'classInstScores', 'categoryScores',
    'categoryInstScores', 'averageScoreClasses', 'averageScoreInstClasses', 'averageScoreCategories', 'averageScoreInstCategories'}."""
    avg = AVG if avg is None else avg
    conf = np.zeros((34, 34), np.int64)
    zero = lambda: {'tp': 0, 'fn': 0, 'tpWeighted': 0.0, 'fnWeighted': 0.0}      # noqa: E731
    inst_stats = {'classes': {n: zero() for n in INSTANCE_CLASSES}, 'categories': {'human': zero(), 'vehicle': zero()}}
    tables = [evaluate_pair(g, i, p, conf, inst_stats, avg, stats) for g, i, p in images]
    have_inst = all(t is not None for t in tables)
    eval_labels = sorted(LABELS)
    not_ignored = [l for l in eval_labels if not LABELS[l][3]]
    class_scores, class_inst = {}, {}
    for l in eval_labels:
        name, _, has_inst, ignore = LABELS[l]
        if ignore:
            class_scores[name] = class_inst[name] = float('nan')
            continue
        tp = int(conf[l, l])
        fn = int(conf[l, :].sum()) - tp
        others = [g for g in not_ignored if g != l]
        fp = int(conf[others, l].sum())
        class_scores[name] = _score(tp, fp, fn)
        if math.isnan(class_scores[name]):
            _bump(stats, 'class_absent')
        if int(conf[[g for g in eval_labels if LABELS[g][3]], l].sum()) > 0:
            _bump(stats, 'prediction_on_ignored_gt')
        if int(conf[l, [p for p in eval_labels if LABELS[p][3]]].sum()) > 0:
            _bump(stats, 'ignored_label_predicted_on_evaluated_gt')
        if has_inst and have_inst:
            s = inst_stats['classes'][name]
            class_inst[name] = _score(s['tpWeighted'], fp, s['fnWeighted'])
            if not math.isnan(class_inst[name]) and class_inst[name] != class_scores[name]:
                _bump(stats, 'iiou_differs_from_iou')
        else:
            class_inst[name] = float('nan')
    cat_scores, cat_inst = {}, {}
    for cat in CATEGORY_ORDER:
        L = [l for l in category_labels(cat) if not LABELS[l][3]]
        if not L:
            cat_scores[cat] = cat_inst[cat] = float('nan')
            continue
        G = [g for g in not_ignored if LABELS[g][1] != cat]
        tp = int(conf[L][:, L].sum())
        fn = int(conf[L, :].sum()) - tp
        fp = int(conf[G][:, L].sum())
        cat_scores[cat] = _score(tp, fp, fn)
        if tp > int(sum(conf[l, l] for l in L)):
            _bump(stats, 'confusion_inside_category')
        if cat in inst_stats['categories'] and have_inst:
            s = inst_stats['categories'][cat]
            cat_inst[cat] = _score(s['tpWeighted'], fp, s['fnWeighted'])
        else:
            cat_inst[cat] = float('nan')
    return {'conf': conf, 'inst': tables, 'inst_stats': inst_stats, 'classScores': class_scores, 'classInstScores': class_inst,
            'categoryScores': cat_scores, 'categoryInstScores': cat_inst, 'averageScoreClasses': score_average(class_scores),
            'averageScoreInstClasses': score_average(class_inst), 'averageScoreCategories': score_average(cat_scores),
            'averageScoreInstCategories': score_average(cat_inst)}
