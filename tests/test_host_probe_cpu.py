"""CPU: the host half of libupsnet_hip -- size / capacity queries and the argument checks in front of every launch -- under
AddressSanitizer and UndefinedBehaviorSanitizer.

`upsnet_amd.build.build(host_sanitize=True)` builds a second, separately cached library whose host code is instrumented (device code
unchanged); tools/host_probe.cpp, a program of its own, links it and calls only entry points that return before any device call.
It runs as a child process with HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES empty: no GPU is opened, nothing is preloaded.
"""
import collections
import functools
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_abi_cpu import header_symbols

pytestmark = pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "hipcc")) is None,
                                reason="hipcc is not installed: the host-instrumented library cannot be built")

QUERY = re.compile(r"_(workspace_bytes|capacity|ints|words|floats|elems|fits|chunk_pixels)$")
PROBE = os.path.join(ROOT, "tools", "host_probe")


def header_text():
    txt = open(os.path.join(ROOT, "include", "upsnet_hip.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def launching_entry_points():
    """Every declaration that takes a stream, and the `_nms` drop-in (host pointers, launches on the null stream)."""
    protos = re.findall(r"\b(upsnet_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header_text(), flags=re.S)
    return sorted({n for n, args in protos if re.search(r"\bvoid \*stream\b", args)} | {"upsnet_nms_host"})


@functools.lru_cache(maxsize=None)
def probe_output():
    from upsnet_amd import build
    lib = build.build(verbose=False, host_sanitize=True)
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    src = os.path.join(ROOT, "tools", "host_probe.cpp")
    if not os.path.exists(PROBE) or os.path.getmtime(PROBE) < max(os.path.getmtime(src), os.path.getmtime(lib)):
        # plain host C++ (-x c++: no device code is generated at all); -fno-gpu-sanitize states it for the driver as well
        subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-fno-gpu-sanitize",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(rocm, "include"),
                               src, "-o", PROBE, "-L" + os.path.dirname(lib), "-lupsnet_hip_hostsan", "-L" + os.path.join(rocm, "lib"),
                               "-lamdhip64", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.join(rocm, "lib")])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    pr = subprocess.run([PROBE], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL)
    out, err = pr.stdout.decode(), pr.stderr.decode(errors="replace")
    # a sanitizer report ends the probe (-fno-sanitize-recover=all): its text is the failure message
    assert pr.returncode == 0 and not err, "host_probe: exit %d after %d lines\n%s" % (pr.returncode, out.count("\n"), err[-4000:])
    assert "BAD " not in out, [l for l in out.splitlines() if l.startswith("BAD ")]
    queries, refusals = [], []
    for line in out.splitlines():
        if line.startswith("Q "):
            m = re.match(r"Q (\w+) (\w+) ([01]) (\S*) -> (-?\d+)$", line)
            assert m, line
            args = tuple(int(a) for a in m.group(4).split(",")) if m.group(4) else ()
            queries.append(("upsnet_" + m.group(1), m.group(2), int(m.group(3)), args, int(m.group(5))))
        elif line.startswith("R "):
            m = re.match(r"R (\w+) (\S+) ret=(-?\d+) hip=([01]) msg=(.*)$", line)
            assert m, line
            refusals.append((m.group(1), m.group(2), int(m.group(3)), int(m.group(4)), m.group(5)))
    return queries, refusals


def test_probe_is_clean_and_covers_every_query():
    """No ASan / UBSan report over the whole grid, and a query added to the header without a probe row fails here."""
    queries, _ = probe_output()
    declared = sorted(s for s in header_symbols() if QUERY.search(s))
    assert len(declared) >= 49
    assert sorted({q[0] for q in queries}) == declared


def test_queries_never_shrink_when_an_argument_grows():
    """Within a sweep one size or count argument grows and the others stay: the answer may grow, stay, or drop to the refusal
    value (0; the NMS family's 256-byte floor) and stay there -- never come back as a smaller positive size, which is what a
    product that wrapped looks like."""
    queries, _ = probe_output()
    sweeps = collections.OrderedDict()
    for name, sweep, mono, args, value in queries:
        if mono:
            sweeps.setdefault((name, sweep), []).append((args, value))
    assert len(sweeps) >= 60
    for (name, sweep), rows in sweeps.items():
        floor = min(v for _, v in rows)
        assert floor >= 0, (name, rows)
        best, refused = None, False
        for args, value in rows:
            if refused:
                assert value == floor, "%s%r = %d after a refusal" % (name, args, value)
            elif best is not None and value < best:
                assert value == floor and value in (0, 256), "%s%r = %d, below %d for a smaller argument" % (name, args, value, best)
                refused = True
            else:
                best = value


# Documented limits: one above the maximum, a negative count, or an image beyond the pixel limit answers 0 ("refused"), never a size.
REFUSED = [
    ("upsnet_pq_workspace_bytes", (4097,)), ("upsnet_pq_workspace_bytes", (-1,)),                              # PQ_MAX_GT = 4096
    ("upsnet_pq_boundary_workspace_bytes", (4097, 64, 96)), ("upsnet_pq_boundary_workspace_bytes", (100, 46341, 46341)),   # H * W >= 2^31
    ("upsnet_pan_boundary_workspace_bytes", (46341, 46341)), ("upsnet_pan_boundary_workspace_bytes", (0, 96)),
    ("upsnet_cs_inst_counts_ints", (65536,)), ("upsnet_cs_inst_workspace_bytes", (65536,)), ("upsnet_cs_inst_workspace_bytes", (-1,)),
    ("upsnet_gt_prepare_workspace_bytes", (0,)), ("upsnet_gt_prepare_workspace_bytes", (65537,)),
    ("upsnet_vis_workspace_bytes", (257, 64, 96)), ("upsnet_vis_workspace_bytes", (10, 46341, 46341)),
    ("upsnet_pan_track_workspace_bytes", (4096, 4097)), ("upsnet_pan_track_table_ints", (4096, 4097)),         # H * W > 2^24
    ("upsnet_pan_track_motion_workspace_bytes", (4096, 4097)), ("upsnet_pan_components_workspace_bytes", (4096, 4097)),
    ("upsnet_pan_absorb_workspace_bytes", (4096, 4097)),
    ("upsnet_video_eval_workspace_bytes", (4097, 64, 96, 2)), ("upsnet_video_eval_workspace_bytes", (100, 64, 96, 9)),
    ("upsnet_video_eval_workspace_bytes", (100, 4096, 4097, 2)), ("upsnet_mots_eval_workspace_bytes", (4097, 64, 96)),
    ("upsnet_mots_eval_workspace_bytes", (100, 4096, 4097)),
    ("upsnet_poly_raster_workspace_bytes", (100, (1 << 24) + 1)), ("upsnet_poly_raster_workspace_bytes", (-1, 5)),
    ("upsnet_combined_pan_workspace_bytes", (0, 1 << 20)), ("upsnet_combined_pan_workspace_bytes", (4, -1)),
    ("upsnet_proposal_recall_workspace_bytes", (0, 1 << 20)), ("upsnet_det_eval_accumulate_workspace_bytes", (-1, 100)),
    ("upsnet_det_eval_image_workspace_bytes", (100, 100, 50, 0, 96, 1)), ("upsnet_boundary_masks_workspace_bytes", (10, 0, 96)),
    ("upsnet_dcn_packed_weight_floats", (0, 256, 3, 3)), ("upsnet_dcn_packed_weight_bf16_elems", (-1, 256, 3, 3)),
    ("upsnet_conv1x1_ksw_packed_weight_floats", (-1, 1)), ("upsnet_conv3x3_ksw_packed_weight_floats", (-1,)),
    ("upsnet_deform_conv_fused_splitk_workspace_bytes", (64, 96, 256, 3, 3, 1, 0, 1, 4)),                     # stride 0
    ("upsnet_deform_conv_fused_splitk_workspace_bytes", (0, 96, 256, 3, 3, 1, 1, 1, 4)),
    ("upsnet_conv2d_splitk_workspace_bytes", (2, 64, 96, 256, 3, 3, 0, 1, 4)), ("upsnet_conv2d_splitk_workspace_bytes", (2, 0, 96, 256, 3, 3, 1, 1, 4)),
    ("upsnet_proposal_workspace_bytes", (9, 64, 64, 3, 1000, 1000)), ("upsnet_proposal_workspace_bytes", (5, 46341, 46341, 3, 1000, 1000)),
    ("upsnet_proposal_workspace_bytes", (5, -1, -1, 3, 1000, 1000)),
    ("upsnet_group_norm_workspace_bytes", (6, 1, 64, 96)), ("upsnet_group_norm_workspace_bytes", (1, 1, -1, 4)),
    ("upsnet_boundary_dilation_fits", (0, 96, 2)),
    ("upsnet_mask_roi_capacity", (2147483647, 2147483647, 0)),                                                  # beyond an int: no capacity
]


def test_documented_limits_are_refused_not_wrapped():
    queries, _ = probe_output()
    table = {(name, args): value for name, _, _, args, value in queries}
    for key in REFUSED:
        assert key in table, "tools/host_probe.cpp has no row %s%r" % key
        assert table[key] == 0, "%s%r = %d: a size where the contract says refused" % (key + (table[key],))
    # and in-contract answers are what they were (tests/test_abi_cpu.py pins the same numbers through ctypes)
    assert table[("upsnet_mask_roi_capacity", (1000, 9, 0))] == 8000 and table[("upsnet_mask_roi_capacity", (1000, 9, 1))] == 8000
    assert table[("upsnet_nms_workspace_bytes", (5, 1000))] > 5 * 1000 * 16 * 8
    assert table[("upsnet_pan_boundary_workspace_bytes", (46340, 46341))] == 46340 * 46341
    assert table[("upsnet_conv2d_splitk_workspace_bytes", (2, 64, 96, 256, 3, 3, 1, 1, 4))] == 4 * 2 * 64 * 96 * 256 * 4


# what each out-of-contract row must be refused FOR: the refusal text, not merely a non-zero return
EXPECT = {
    "null": None,                                        # every argument zero: any refusal that names the entry point
    # the pointer check itself. null_ptr: sizes with which the same call with NON-null pointers passed every argument check (it got
    # as far as the runtime), every pointer null: whatever the refusal says, it can only be for the pointers. null_ptr_msg: no such
    # sizes were found (sizes of 1): the message itself must speak of the pointer, unless the launcher also has a null_ptr row.
    "null_ptr": None,
    "null_ptr_msg": None,
    "bad_dim": None,                                     # every pointer non-null, every size -1: any refusal (a size check exists)
    "cin_not_32": r"multiple of 32|% 32",
    "ldw_below_cout": r"ldw",
    "empty_output": r"empty output",
    # conv_fill's limits (csrc/conv_params.h), at exactly 2^30 input floats / 2^29 output floats
    "input_2^30": r"feature map \d+ exceeds 4 GiB \(32-bit byte offsets\)",
    "output_2^29": r"output \d+ exceeds 2 GiB \(32-bit byte offsets in the epilogue\)",
    # a launcher's own tighter limit, on a row that conv_fill lets through: the launcher's own wording
    "own_input": r"feature map( \d+)? exceeds [12] GiB; split the batch|image batch too large",
    "own_output": r"output exceeds 2 GiB; split the batch",
    "input_huge": r"feature map( \d+)? exceeds [24] GiB|image batch too large",     # launchers that do not go through conv_fill's rows above
    "image_2^31": r"46341 ?x ?46341",
    "image_limit": r"1048576 x 1048576|32768 x 32768",
    "below_limit": None,                                 # one step inside the limit: NOT refused for its size (see the test)
}
SIZE_REFUSAL = re.compile(r"exceeds|too large|bad (image|frame|map|output|sizes)")
# launchers whose own size guard must have a row (the guard's file in brackets)
OWN_INPUT = ["upsnet_deform_conv_fused_nhwc", "upsnet_deform_conv_fused_nhwc_bf16", "upsnet_conv2d_nhwc_bf16", "upsnet_conv1x1_frag_nhwc_f32",
             "upsnet_conv1x1_frag_nhwc_f32_splitk", "upsnet_conv1x1_siblings_nhwc_f32", "upsnet_deconv2x2_frag_nhwc_f32",
             "upsnet_conv2d_winograd_nhwc_f32_tail", "upsnet_bottleneck_bf16", "upsnet_bottleneck_proj_bf16", "upsnet_stem_pool_bf16"]
IMAGE_GUARDED = ["upsnet_pq_accumulate", "upsnet_pan_boundary_map", "upsnet_pq_boundary_accumulate", "upsnet_det_eval_image",
                 "upsnet_det_eval_boundary_image", "upsnet_boundary_masks", "upsnet_poly_raster", "upsnet_pan_format", "upsnet_pan_relabel",
                 "upsnet_pan_stable_colors", "upsnet_cs_inst_image", "upsnet_cs_pixel_image", "upsnet_cs_inst_expand", "upsnet_gt_prepare",
                 "upsnet_video_eval_frame", "upsnet_mots_eval_frame", "upsnet_pan_track_step", "upsnet_pan_components"]


def test_every_launcher_refuses_bad_arguments_before_any_device_call():
    """There is no GPU here, so an entry point that fails to refuse gets a HIP error from its launch: that must not pass as a
    refusal. hip=1 marks a message that carries a HIP runtime error string."""
    _, refusals = probe_output()
    launchers = launching_entry_points()
    for tag in ("null", "bad_dim"):
        assert sorted({r[0] for r in refusals if r[1] == tag}) == launchers, tag
    proven = {r[0] for r in refusals if r[1] == "null_ptr"}
    assert sorted(proven | {r[0] for r in refusals if r[1] == "null_ptr_msg"}) == launchers
    assert len(proven) >= 90
    assert {r[1] for r in refusals} == set(EXPECT)
    by_tag = collections.defaultdict(set)
    for name, tag, ret, hip, msg in refusals:
        by_tag[tag].add(name)
        where = "%s [%s]: ret=%d hip=%d msg=%r" % (name, tag, ret, hip, msg)
        if tag == "below_limit":
            # the row passes every argument check and reaches the runtime, which has no device: a `<` turned into `<=` shows here
            assert ret != 0 and hip and not SIZE_REFUSAL.search(msg), where
            continue
        if name in ("upsnet_zero_fill", "upsnet_proposal_recall") and tag == "null" and ret == 0:
            continue          # their all-zero call is the documented no-op; the row after it (16 bytes / one problem) is the refusal
        if name == "upsnet_zero_fill" and tag == "bad_dim":
            continue          # its only size is a size_t byte count: every value is in contract
        assert ret != 0 and msg and not hip, where
        who = msg.split(":")[0]
        # ... by the entry point's own name, or by that of the launcher it shares with its siblings, whose words are a part of
        # its own (pyramid_proposals for _strided_ordered) or which its own words are a part of (soft_nms_batched for soft_nms)
        mine, named = set(name.replace("upsnet_", "").split("_")), set(who.replace("upsnet_", "").split("_"))
        assert re.fullmatch(r"[a-z0-9_]+", who) and (named <= mine or mine <= named), "the message does not name the entry point: " + where
        if EXPECT[tag]:
            assert re.search(EXPECT[tag], msg), where
        if tag == "null_ptr_msg" and name not in proven:
            assert re.search(r"null|NULL|given", msg), where
    for name in ("upsnet_zero_fill", "upsnet_proposal_recall"):
        assert [r for r in refusals if r[0] == name and r[2] != 0 and "null pointer" in r[4]], name
    assert set(OWN_INPUT) <= by_tag["own_input"], sorted(set(OWN_INPUT) - by_tag["own_input"])
    assert set(IMAGE_GUARDED) <= by_tag["image_2^31"], sorted(set(IMAGE_GUARDED) - by_tag["image_2^31"])
    assert len(by_tag["below_limit"]) >= 6
