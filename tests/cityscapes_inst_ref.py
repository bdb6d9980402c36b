"""Numpy restatement of the Cityscapes devkit's instance-level evaluation (evalInstanceLevelSemanticLabeling, default arguments) on
FULL boolean masks, for the tests of dataset/cityscapes_eval.py: `gtNp == id` arrays, np.logical_and, np.count_nonzero, the devkit's
loops over dict lists and its np.append order. It shares no code with the product.

A prediction is {'cls': 1..8, 'conf': float, 'mask': bool / uint8 [H, W]}. Deviations restated with the rules: a prediction of zero
area is dropped before matching; a (class, threshold) with GT and predictions but no entry at all has AP 0.0.

`evaluate(images, stats)` fills `stats` (a dict of counters) with how often each branch of the rules was taken."""
import numpy as np

CLASSES = [('person', 24), ('rider', 25), ('car', 26), ('truck', 27), ('bus', 28), ('train', 31), ('motorcycle', 32), ('bicycle', 33)]
VOID_IDS = [0, 1, 2, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18, 29, 30]
OVERLAPS = np.arange(0.5, 1.0, 0.05)
MIN_REGION_SIZE = 100


def match_image(gt_np, preds):
    """assignGt2Preds for one image: ({class name: GT instance dicts}, {class name: prediction dicts}, integer counts per prediction).
    counts[i] = None for a dropped prediction, else {'area', 'void', 'inter': {raw value: pixels}}."""
    gt_instances = {name: [] for name, _ in CLASSES}
    for v in np.unique(gt_np):
        v = int(v)
        label_id = v // 1000 if v >= 1000 else v
        inst = {'instID': v, 'labelID': label_id, 'pixelCount': int(np.count_nonzero(gt_np == v)), 'matchedPred': []}
        for name, lid in CLASSES:
            if lid == label_id:
                gt_instances[name].append(inst)
    pred_instances = {name: [] for name, _ in CLASSES}
    void = np.zeros(gt_np.shape, bool)
    for lid in VOID_IDS:
        void = np.logical_or(void, gt_np == lid)
    counts = []
    for pred_id, p in enumerate(preds):
        mask = np.not_equal(p['mask'], 0)
        pixel_count = int(np.count_nonzero(mask))
        if pixel_count == 0:
            counts.append(None)
            continue
        name = CLASSES[p['cls'] - 1][0]
        pred = {'predID': pred_id, 'pixelCount': pixel_count, 'confidence': float(p['conf']),
                'voidIntersection': int(np.count_nonzero(np.logical_and(void, mask))), 'matchedGt': []}
        inter = {}
        for gt in gt_instances[name]:
            intersection = int(np.count_nonzero(np.logical_and(gt_np == gt['instID'], mask)))
            if intersection > 0:
                gt_copy = {k: gt[k] for k in ('instID', 'labelID', 'pixelCount')}
                pred_copy = {k: pred[k] for k in ('predID', 'pixelCount', 'confidence')}
                gt_copy['intersection'] = intersection
                pred_copy['intersection'] = intersection
                pred['matchedGt'].append(gt_copy)
                gt['matchedPred'].append(pred_copy)
                inter[gt['instID']] = intersection
        pred_instances[name].append(pred)
        counts.append({'area': pixel_count, 'void': pred['voidIntersection'], 'inter': inter})
    return gt_instances, pred_instances, counts


def _bump(stats, key, n=1):
    if stats is not None:
        stats[key] = stats.get(key, 0) + n


def average_precision(y_true, y_score, hard_fns):
    score_arg_sort = np.argsort(y_score)
    y_score_sorted = y_score[score_arg_sort]
    y_true_sorted = y_true[score_arg_sort]
    y_true_sorted_cumsum = np.cumsum(y_true_sorted)
    (thresholds, unique_indices) = np.unique(y_score_sorted, return_index=True)
    nb_prec_recall = len(unique_indices) + 1
    nb_examples = len(y_score_sorted)
    nb_true_examples = y_true_sorted_cumsum[-1] if nb_examples > 0 else 0.0
    precision = np.zeros(nb_prec_recall)
    recall = np.zeros(nb_prec_recall)
    y_true_sorted_cumsum = np.append(y_true_sorted_cumsum, 0)
    for idx_res, idx_scores in enumerate(unique_indices):
        cum_sum = y_true_sorted_cumsum[idx_scores - 1]
        tp = nb_true_examples - cum_sum
        fp = nb_examples - idx_scores - tp
        fn = cum_sum + hard_fns
        p = float(tp) / (tp + fp)
        r = float(tp) / (tp + fn)
        precision[idx_res] = p
        recall[idx_res] = r
    precision[-1] = 1.
    recall[-1] = 0.
    recall_for_conv = np.copy(recall)
    recall_for_conv = np.append(recall_for_conv[0], recall_for_conv)
    recall_for_conv = np.append(recall_for_conv, 0.)
    step_widths = np.convolve(recall_for_conv, [-0.5, 0, 0.5], 'valid')
    return np.dot(precision, step_widths)


def evaluate_matches(matches, stats=None):
    """evaluateMatches: matches = [(gt_instances, pred_instances)] per image -> aps float64 [8, 10]."""
    aps = np.zeros((len(CLASSES), len(OVERLAPS)))
    for li, (label_name, _) in enumerate(CLASSES):
        for oi, overlap_th in enumerate(OVERLAPS):
            y_true = np.empty(0)
            y_score = np.empty(0)
            y_image = np.empty(0)
            hard_fns = 0
            have_gt = False
            have_pred = False
            for image_index, (gt_all, pred_all) in enumerate(matches):
                pred_instances = pred_all[label_name]
                gt_instances = [gt for gt in gt_all[label_name] if gt['instID'] >= 1000 and gt['pixelCount'] >= MIN_REGION_SIZE]
                if gt_instances:
                    have_gt = True
                if pred_instances:
                    have_pred = True
                cur_true = np.ones(len(gt_instances))
                cur_score = np.ones(len(gt_instances)) * (-float('inf'))
                cur_match = np.zeros(len(gt_instances), dtype=bool)
                for gt_i, gt in enumerate(gt_instances):
                    found_match = False
                    for pred in gt['matchedPred']:
                        overlap = float(pred['intersection']) / (gt['pixelCount'] + pred['pixelCount'] - pred['intersection'])
                        if overlap > overlap_th:
                            confidence = pred['confidence']
                            if cur_match[gt_i]:
                                max_score = max(cur_score[gt_i], confidence)
                                min_score = min(cur_score[gt_i], confidence)
                                cur_score[gt_i] = max_score
                                cur_true = np.append(cur_true, 0)
                                cur_score = np.append(cur_score, min_score)
                                cur_match = np.append(cur_match, True)
                                _bump(stats, 'duplicate_matchers')
                            else:
                                found_match = True
                                cur_match[gt_i] = True
                                cur_score[gt_i] = confidence
                    if not found_match:
                        hard_fns += 1
                        _bump(stats, 'hard_false_negatives')
                cur_true = cur_true[cur_match == True]      # noqa: E712  (the devkit's spelling)
                cur_score = cur_score[cur_match == True]    # noqa: E712
                for pred in pred_instances:
                    found_gt = False
                    for gt in pred['matchedGt']:
                        overlap = float(gt['intersection']) / (gt['pixelCount'] + pred['pixelCount'] - gt['intersection'])
                        if overlap > overlap_th:
                            found_gt = True
                            if not (gt['instID'] >= 1000 and gt['pixelCount'] >= MIN_REGION_SIZE):
                                _bump(stats, 'matched_only_non_valid')
                            break
                    if not found_gt:
                        nb_ignore_pixels = pred['voidIntersection']
                        if pred['voidIntersection'] > 0:
                            _bump(stats, 'void_intersections')
                        for gt in pred['matchedGt']:
                            if gt['instID'] < 1000:
                                nb_ignore_pixels += gt['intersection']
                                _bump(stats, 'group_intersections')
                            if gt['pixelCount'] < MIN_REGION_SIZE:
                                nb_ignore_pixels += gt['intersection']
                                _bump(stats, 'small_gt_intersections')
                        proportion_ignore = float(nb_ignore_pixels) / pred['pixelCount']
                        if proportion_ignore <= overlap_th:
                            cur_true = np.append(cur_true, 0)
                            cur_score = np.append(cur_score, pred['confidence'])
                            _bump(stats, 'false_positives')
                        else:
                            _bump(stats, 'ignored_predictions')
                y_true = np.append(y_true, cur_true)
                y_score = np.append(y_score, cur_score)
                y_image = np.append(y_image, np.full(len(cur_score), image_index))
            if stats is not None and len(y_score):
                for s in np.unique(y_score):
                    if len(np.unique(y_image[y_score == s])) > 1:
                        _bump(stats, 'tied_scores_across_images')
            if have_gt and have_pred:
                ap_current = average_precision(y_true, y_score, hard_fns)
                _bump(stats, 'ap_curve')
            elif have_gt:
                ap_current = 0.0
                _bump(stats, 'ap_zero')
            else:
                ap_current = float('nan')
                _bump(stats, 'ap_nan_with_pred' if have_pred else 'ap_nan')
            aps[li, oi] = ap_current
    return aps


def compute_averages(aps):
    """computeAverages: {'AP', 'AP50', 'per_class': {name: {'ap', 'ap50'}}}."""
    import warnings
    d50 = np.where(np.isclose(OVERLAPS, 0.5))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        res = {'AP': np.nanmean(aps[:, :]), 'AP50': np.nanmean(aps[:, d50]), 'per_class': {}}
        for li, (name, _) in enumerate(CLASSES):
            res['per_class'][name] = {'ap': np.average(aps[li, :]), 'ap50': np.average(aps[li, d50])}
    return res


def evaluate(images, stats=None):
    """images = [(gt_np uint16 [H, W], predictions)] -> (aps [8, 10], averages dict, per-image prediction counts)."""
    matches, counts = [], []
    for gt_np, preds in images:
        g, p, c = match_image(gt_np, preds)
        matches.append((g, p))
        counts.append(c)
    aps = evaluate_matches(matches, stats)
    return aps, compute_averages(aps), counts
