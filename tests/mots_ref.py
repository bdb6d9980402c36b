"""Plain numpy restatement of the MOTS measures of include/upsnet_hip.h (Voigtlaender et al., CVPR 2019: sMOTSA, MOTSA, MOTSP, IDS, Frag,
MT / PT / ML): dicts, Python ints and loops over the (GT row, pred key) pairs that np.unique finds per frame. The yardstick of
tests/test_mots_*.py and the builders of their cases. Nothing here is shared with the evaluator under test; like it, this restates the
published definitions and was never compared with a build of mots_tools."""
import numpy as np

import video_pq_ref as vref

VOID = 255
COUNTS = ('tp', 'fp', 'fn', 'gt_masks', 'ids', 'frag', 'fp_ignored', 'mt', 'pt', 'ml')


def gt_ids(gt):
    return gt[:, :, 0].astype(np.int64) + 256 * gt[:, :, 1].astype(np.int64) + 65536 * gt[:, :, 2].astype(np.int64)


def pred_keys(pred):
    """category << 8 | instance per pixel, -1 for pred VOID."""
    key = (pred[:, :, 0].astype(np.int64) << 8) | pred[:, :, 1].astype(np.int64)
    key[pred[:, :, 0] == VOID] = -1
    return key


class RefMOTSEvaluator(object):
    def __init__(self, categories):
        self.categories = categories if isinstance(categories, dict) else {el['id']: el for el in categories}
        self.things = sorted(c for c, el in self.categories.items() if el['isthing'] == 1)
        for name in COUNTS:
            setattr(self, name, {})
        self.soft = {}                  # float64 sums in the stated order
        self.sequences = 0
        self.frames = 0

    def _inc(self, name, c, v=1):
        d = getattr(self, name)
        d[c] = d.get(c, 0) + v

    def add_sequence(self, preds, gts, frames_segments_info):
        rows = {}
        for segs in frames_segments_info:
            for s in segs:
                rows[int(s['id'])] = (int(s['category_id']), int(s.get('iscrowd', 0)))
        state = {gid: {'last': None, 'gap': False, 'present': 0, 'tracked': 0} for gid in rows}
        for pred, gt in zip(preds, gts):
            key, gid = pred_keys(pred).reshape(-1), gt_ids(gt).reshape(-1)
            for c in np.unique(key[key >= 0] >> 8).tolist():
                if c not in self.categories:
                    raise KeyError(c)
            pairs, cnt = np.unique(np.stack([gid, key]), axis=1, return_counts=True)
            joint, area_p, area_g = {}, {}, {}
            for (g, k), v in zip(pairs.T.tolist(), cnt.tolist()):
                joint[(g, k)] = v
                area_p[k] = area_p.get(k, 0) + v
                area_g[g] = area_g.get(g, 0) + v
            for c in self.things:
                objects = sorted(g for g, (cat, crowd) in rows.items() if cat == c and not crowd)
                ignore = [g for g in area_g if g == 0 or g not in rows or rows[g] == (c, 1)]
                hyps = sorted(k for k in area_p if k >= 0 and k >> 8 == c)
                matched = {}
                for g in objects:                                   # ascending id
                    partners = [k for k in hyps if 3 * joint.get((g, k), 0) > area_g.get(g, 0) + area_p[k]]
                    assert len(partners) <= 1
                    if area_g.get(g, 0) == 0:
                        continue
                    st = state[g]
                    st['present'] += 1
                    self._inc('gt_masks', c)
                    if not partners:
                        self._inc('fn', c)
                        if st['last'] is not None:
                            st['gap'] = True
                        continue
                    k = partners[0]
                    assert k not in matched.values()
                    matched[g] = k
                    inter = joint[(g, k)]
                    self._inc('tp', c)
                    self.soft[c] = self.soft.get(c, 0.0) + float(inter) / float(area_g[g] + area_p[k] - inter)
                    st['tracked'] += 1
                    if st['last'] is not None and st['last'] != k:
                        self._inc('ids', c)
                    st['last'] = k
                    if st['gap']:
                        self._inc('frag', c)
                        st['gap'] = False
                for k in hyps:
                    if k in matched.values():
                        continue
                    ign = sum(joint.get((g, k), 0) for g in ignore)
                    self._inc('fp_ignored' if 2 * ign > area_p[k] else 'fp', c)
        for g, st in state.items():
            c, crowd = rows[g]
            if crowd or c not in self.things or st['present'] == 0:
                continue
            if 5 * st['tracked'] > 4 * st['present']:
                self._inc('mt', c)
            elif 5 * st['tracked'] < st['present']:
                self._inc('ml', c)
            else:
                self._inc('pt', c)
        self.sequences += 1
        self.frames += len(preds)

    def vector(self, name):
        out = np.zeros(256, np.float64 if name == 'soft' else np.int64)
        for c, v in getattr(self, name).items():
            out[c] = v
        return out

    def figures(self, c):
        g = lambda name: getattr(self, name).get(c, 0)     # noqa: E731
        gt, tp, soft = max(g('gt_masks'), 1), g('tp'), self.soft.get(c, 0.0)
        return {'motsa': float(tp - g('fp') - g('ids')) / gt, 'smotsa': (soft - g('fp') - g('ids')) / gt, 'motsp': soft / max(tp, 1),
                'recall': float(tp) / gt, 'precision': float(tp) / max(tp + g('fp'), 1)}

    def mean(self):
        scored = [self.figures(c) for c in self.things if self.gt_masks.get(c, 0) > 0]
        out = {k: (sum(r[k] for r in scored) / len(scored) if scored else 0.0) for k in ('smotsa', 'motsa', 'motsp', 'recall', 'precision')}
        out['n'] = len(scored)
        return out


# ------------------------------------------------------------------------------------------------ run-length encoding, restated
def rle_counts(mask):
    """pycocotools' counts of a boolean [H,W] mask: run lengths over the column-major flattening, starting with the zeros."""
    flat = np.asarray(mask, bool).T.reshape(-1)
    counts, run, value = [], 0, False
    for v in flat.tolist():
        if v != value:
            counts.append(run)
            run, value = 0, v
        run += 1
    counts.append(run)
    return counts


def thing_segments(pan):
    """{category << 8 | instance: mask} of the thing segments (category != 255, instance >= 1) of a 2-channel map."""
    key = pred_keys(pan)
    return {k: key == k for k in np.unique(key).tolist() if k >= 0 and k & 255}


def transitions(mask):
    """The column-major positions at which the membership changes (none reported at H * W)."""
    counts = rle_counts(mask)
    return np.cumsum(counts)[:-1].tolist()


def mots_lines(maps_2ch, to_string):
    """The lines write_mots_txt writes, from the masks alone (to_string: the counts -> compressed string routine)."""
    lines = []
    for t, m in enumerate(maps_2ch):
        H, W = m.shape[:2]
        for k, mask in sorted(thing_segments(m).items()):
            lines.append('%d %d %d %d %d %s' % (t, (k >> 8) * 1000 + (k & 255), k >> 8, H, W, to_string(rle_counts(mask))))
    return lines


# ------------------------------------------------------------------------------------------------ builders
CATEGORIES = vref.CATEGORIES


def knock_out(pred, cat, inst):
    m = (pred[:, :, 0] == cat) & (pred[:, :, 1] == inst)
    pred[m, 0], pred[m, 1] = VOID, 0


def blob_sequence(seed, H, W, frames, switch_at=None):
    """video_pq_ref.blob_sequence (drifting rectangles of thing categories 1, 2, 11 on two stuff halves, a crowd object, a GT VOID band,
    an id outside the table, a wrong-category prediction, an identity switch of object 1 at `switch_at`) with two tracker failures:
    object 2 (category 2) is not predicted in the middle frame (a gap, then a resumption) and object 5 (category 2) is predicted in
    the first frame only (mostly lost)."""
    preds, gts, infos = vref.blob_sequence(seed, H, W, frames, switch_at=switch_at)
    for t, p in enumerate(preds):
        if t == frames // 2:
            knock_out(p, 2, 2)
        if t > 0:
            knock_out(p, 2, 5)
    return preds, gts, infos


# the blob sequences of tests/test_mots_gpu.py at 48 x 64: tests/test_mots_cpu.py asserts that they hold every kind of event
GPU_BLOBS = [(3, 48, 64, 6, 2), (4, 48, 64, 6, 3)]


def seg(gid, cat, crowd=0):
    return vref.seg(gid, cat, crowd)


def strip_case(pred_spec, gt_spec, segs, W=12):
    """One-row frames from interval lists: pred_spec / gt_spec are per frame lists of (category, instance, x0, x1) / (id, x0, x1),
    inclusive; pred VOID and GT background id 900 (stuff 200) elsewhere. -> (preds, gts, infos); segs: per frame, or one list for all."""
    preds, gts, infos = [], [], []
    for t, (ps, gs) in enumerate(zip(pred_spec, gt_spec)):
        p, g = vref.blank_pred(1, W), vref.blank_gt(1, W)
        vref.put_gt(g, 900, 0, 0, 0, W - 1)
        for gid, x0, x1 in gs:
            vref.put_gt(g, gid, 0, 0, x0, x1)
        for cat, inst, x0, x1 in ps:
            vref.put_pred(p, cat, inst, 0, 0, x0, x1)
        preds.append(p)
        gts.append(g)
        infos.append(list(segs[t] if segs and isinstance(segs[0], list) else segs) + [seg(900, 200)])
    return preds, gts, infos
