"""CPU: tests/pan_confidence_ref.py (the restatement the device is held to in tests/test_pan_confidence_gpu.py) against literals
worked out by hand, and the claim about the GPU test's inputs that makes its bound mean something: on conf_crowd, summing only the
first of the instances that touch a tile nowhere -- the arg-max's shortcut carried over to the softmax -- moves the confidence by far
more than the tolerance."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pan_confidence_ref as ref  # noqa: E402

F32 = np.float32


def _planes(stuff, thing, seg_inst, energy):
    """One pixel: fcn_output [S,1,1] = stuff | thing channels, seg_inst / mask_energy [k,1,1]."""
    fcn = np.asarray(list(stuff) + list(thing), F32).reshape(-1, 1, 1)
    return fcn, np.asarray(seg_inst, F32).reshape(-1, 1, 1), np.asarray(energy, F32).reshape(-1, 1, 1), len(stuff)


def test_stuff_pixel_with_the_dummy_instance():
    # stuff logits (ln 3, 0); the dummy instance channel is 0; one thing channel ln 2, so void = ln 2 - max_j seg_inst_j = ln 2 - 0.
    # exp: 3 + 1 | 1 | 2 = 7. Winner: stuff channel 0 with P = 3/7. 255 * 3/7 = 109.2857..., + 0.5 truncates to 109.
    conf, win = ref.confidence(*_planes([math.log(3), 0.0], [math.log(2)], [0.0], [0.0]))
    assert win[0, 0] == 0
    assert abs(conf[0, 0] - 3 / 7) < 1e-7          # (the logits are fp32: ln 3 carries 2^-24 of relative error)
    assert ref.quantize(conf)[0, 0] == 109


def test_pixel_won_by_an_instance():
    # stuff (0, 0); instance 0: seg_inst = ln 2 (its thing channel), mask energy ln 2, logit ln 4; void = ln 2 - ln 2 = 0.
    # exp: 1 + 1 | 4 | 1 = 7. Winner: channel 2 = s_stuff + 0 with P = 4/7. 255 * 4/7 = 145.714..., + 0.5 truncates to 146.
    ln2 = F32(math.log(2))
    conf, win = ref.confidence(*_planes([0.0, 0.0], [ln2], [ln2], [ln2]))
    assert win[0, 0] == 2
    assert abs(conf[0, 0] - 4 / 7) < 1e-6          # (ln 2 + ln 2 is rounded to fp32 once more)
    assert ref.quantize(conf)[0, 0] == 146


def test_void_pixel():
    # stuff (0, 0); two instances that do not reach the pixel (seg_inst 0, energy 0, logit 0 each); thing channels (ln 5, -1):
    # void = ln 5 - 0. exp: 1 + 1 | 1 + 1 | 5 = 9. Winner: void (255) with P = 5/9. 255 * 5/9 = 141.666..., + 0.5 truncates to 142.
    conf, win = ref.confidence(*_planes([0.0, 0.0], [math.log(5), -1.0], [0.0, 0.0], [0.0, 0.0]))
    assert win[0, 0] == 255
    assert abs(conf[0, 0] - 5 / 9) < 1e-7
    assert ref.quantize(conf)[0, 0] == 142


def test_every_untouched_instance_counts():
    # stuff (0,); five instances at 0; thing channel 0 -> void = 0: seven logits of 0, P[winner] = 1/7 (winner: stuff channel 0, the
    # first maximum). With only the first zero instance: three logits, 1/3.
    fcn, si, en, s = _planes([0.0], [0.0], [0.0] * 5, [0.0] * 5)
    conf, win = ref.confidence(fcn, si, en, s)
    assert win[0, 0] == 0 and abs(conf[0, 0] - 1 / 7) < 1e-15
    wrong, _ = ref.confidence(fcn, si, en, s, first_zero_only=True)
    assert abs(wrong[0, 0] - 1 / 3) < 1e-15


def test_quantisation_around_every_byte():
    # q = (unsigned)(conf * 255.0f + 0.5f): conf = k/255 and its fp32 neighbours on both sides all give k (the half-way points
    # (k + 0.5)/255 are about 2^15 ulps away).
    k = np.arange(256)
    c = (k / 255.0).astype(F32)
    assert np.array_equal(ref.quantize(c), k)
    assert np.array_equal(ref.quantize(np.nextafter(c, F32(2))[:-1]), k[:-1])
    assert np.array_equal(ref.quantize(np.nextafter(c, F32(-1))[1:]), k[1:])
    # just below / above a half-way point: 0.5/255 = 0.00196078...; fp32(0.0019607) * 255 + 0.5 < 1 -> 0, fp32(0.0019609) -> 1
    assert ref.quantize(F32(0.0019607)) == 0 and ref.quantize(F32(0.0019609)) == 1
    assert ref.quantize(F32(1.0)) == 255 and ref.quantize(F32(0.0)) == 0


def _two_segments():
    # 2 x 4 map: key (3, 0) on the first three pixels of row 0, key (12, 7) on row 1, one VOID pixel.
    pan = np.zeros((2, 4, 3), np.uint8)
    pan[0, :3] = (3, 0, 0)
    pan[0, 3] = (255, 0, 0)
    pan[1, :] = (12, 7, 0)
    conf = np.asarray([[255, 0, 45, 99], [128, 127, 128, 127]], np.uint8)
    return pan, conf


def test_segment_scores_of_two_segments():
    # (3, 0): area 3, sum 255 + 0 + 45 = 300, score 300 / 765 = 0.39215...; (12, 7): area 4, sum 128 + 127 + 128 + 127 = 510,
    # score 510 / 1020 = 0.5 exactly. The VOID pixel (confidence 99) is in no row.
    pan, conf = _two_segments()
    assert ref.segment_scores(pan, conf) == {(3, 0): (3, 300, 300 / 765.0), (12, 7): (4, 510, 0.5)}
    assert ref.score_table(pan, conf).tolist() == [[3 << 8, 3, 300], [12 << 8 | 7, 4, 510]]
    assert ref.score_table(pan, conf).dtype == np.uint32


def test_filter_is_strict_at_the_threshold():
    pan, conf = _two_segments()
    void = np.asarray((255, 0, 0), np.uint8)
    # T = 0.5: 0.5 * 255 * 4 = 510.0 and sum_q = 510: 510 < 510 is false, (12, 7) stays; 300 < 0.5 * 765 = 382.5: (3, 0) goes.
    out = ref.score_filter(pan, conf, 0.5)
    assert np.array_equal(out[1], pan[1]) and (out[0] == void).all()
    # one step below: sum_q = 509 < 510.0, (12, 7) goes too
    conf2 = conf.copy()
    conf2[1, 0] = 127
    assert (ref.score_filter(pan, conf2, 0.5) == void).all()
    # T = 0 removes nothing (0 < 0 is false even for a segment of sum 0)
    assert np.array_equal(ref.score_filter(pan, np.zeros_like(conf), 0.0), pan)
    # T = 1 keeps only a segment whose every byte is 255
    pan3 = pan.copy()
    conf3 = conf.copy()
    conf3[1] = 255
    out = ref.score_filter(pan3, conf3, 1.0)
    assert np.array_equal(out[1], pan[1]) and (out[0] == void).all()


def test_the_gpu_cases_tell_a_full_sum_from_the_first_zero_shortcut():
    """conf_crowd: 64 kept instances on 128 x 256, scores in [-1, 1]. In a tile no box reaches, all 64 instance logits are 0 and
    z_max <= 1 (stuff, an instance's 0, or void = max thing - 0): the 63 dropped terms are at least 63 / e of a sum that is at most
    (4 + 64 + 1) e^0 ... so the confidence moves by far more than 100 * TOL."""
    (score, rois5, prob, logit, cls, S, C, H, W), _ = ref.conf_crowd()
    good = ref.head_confidence(score, rois5, prob, logit, cls, S, C)
    assert len(good['keep_inds']) == 64
    bad = ref.head_confidence(score, rois5, prob, logit, cls, S, C, first_zero_only=True)
    moved = np.abs(good['conf'] - bad['conf']).max()
    assert moved > 100 * ref.TOL, moved
    assert moved > 0.1, moved      # (in fact the confidence is several times too large)
