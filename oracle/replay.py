"""oracle.replay -- TEST INFRASTRUCTURE ONLY: record the C calls the wrappers of ``oracle/__init__.py`` make, and replay them in the
stand-alone driver ``oracle/c/orc_replay.c`` (``oracle.build_replay``), which can run under ASan / UBSan where code loaded into
Python cannot.

    with replay.recording() as calls:
        oracle.roi_align_forward(feat, rois, 7, 7, 0.25)     # the ctypes call runs as usual ...
    case = calls[0]                                          # ... and its arguments, outputs and return value are kept
    ret, outs, err = replay.run(oracle.build_replay(True), case, fill=0xA5, threads=1)

The case-file format is documented at the top of ``orc_replay.c``.
"""
import contextlib
import ctypes
import os
import struct
import subprocess
import tempfile

import numpy as np

import oracle

IN, OUT, INOUT, NULL = 0, 1, 2, 3
_DTYPES = [np.float32, np.int32, np.int64, np.uint8, np.float64, np.uint32]
_CODE = {np.dtype(t): i for i, t in enumerate(_DTYPES)}

# C function -> (id in orc_replay.c, {argument index: OUT | INOUT}). Everything else is an input. INOUT: the function's contract
# is to ACCUMULATE into (roi_align_backward, deform_col2im: "grad (accumulated)") or to permute in place (soft_nms) what it is given.
FUNCS = {
    "orc_roi_align_forward": (1, {10: OUT}),
    "orc_deform_im2col": (2, {15: OUT}),
    "orc_roi_align_backward": (3, {10: INOUT}),
    "orc_deform_col2im": (4, {18: INOUT}),
    "orc_deform_col2im_coord": (5, {19: OUT, 20: OUT}),
    "orc_nms_sorted": (6, {4: OUT}),
    "orc_cpu_nms_sorted": (7, {4: OUT}),
    "orc_soft_nms": (8, {0: INOUT, 1: INOUT}),
    "orc_resize_at": (9, {}),
    "orc_resize_bilinear": (10, {4: OUT}),
    "orc_mask_removal": (11, {10: OUT, 11: OUT, 12: OUT}),
    "orc_seg_term": (12, {8: OUT}),
    "orc_panoptic_fuse": (13, {9: OUT, 10: OUT}),
    "orc_upsample_bilinear": (14, {5: OUT}),
    "orc_fcn_score_combine": (15, {5: OUT}),      # as recorded: (nlev, S, H, W, bias, out, part[0] .. part[nlev-1])
    "orc_prep_image": (16, {9: OUT}),
    "orc_set_threads": (17, {}),
}
# the functions that return a value (the others are void: ctypes would hand back whatever the register held)
RETURNS = {"orc_nms_sorted", "orc_cpu_nms_sorted", "orc_soft_nms", "orc_mask_removal", "orc_resize_at"}


class Case(object):
    """One recorded call: `records` [(role, array | None)] in driver argument order, `ret` the ctypes return value (None for a void function), `outputs` the
    OUT / INOUT arrays as the ctypes call left them."""

    def __init__(self, name, records, ret, outputs):
        self.name, self.records, self.ret, self.outputs = name, records, ret, outputs

    def input_bytes(self):
        return sum(a.nbytes for role, a in self.records if role in (IN, INOUT))


class _Ptr(ctypes.c_void_p):
    """What the patched oracle._p returns: the pointer ctypes passes on, plus the array it came from."""
    array = None


def _scalar(v):
    if isinstance(v, ctypes.c_float):
        return np.float32(v.value)
    if isinstance(v, ctypes.c_double):
        return np.float64(v.value)
    if isinstance(v, ctypes.c_uint):
        return np.uint32(v.value)
    if isinstance(v, (int, np.integer)):
        return np.int32(v)
    raise TypeError("oracle.replay: cannot record argument %r" % (v,))


class _Recorder(object):
    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("orc_"):
            return fn
        if name not in FUNCS:
            raise KeyError("oracle.replay.FUNCS has no entry for %s: add it there and to orc_replay.c" % name)
        roles = FUNCS[name][1]

        def call(*args):
            vals = list(args)
            if name == "orc_fcn_score_combine":   # (part[], nlev, S, H, W, bias, out): the wrapper passes raw addresses for part[]
                arr, nlev, S, H, W = vals[:5]
                parts = []
                for l in range(nlev):
                    n = (H >> l) * (W >> l) * S
                    p = _Ptr(arr[l])
                    p.array = np.ctypeslib.as_array((ctypes.c_float * n).from_address(arr[l])).reshape(H >> l, W >> l, S)
                    parts.append(p)
                vals = vals[1:] + parts
            records = []
            for i, v in enumerate(vals):
                if v is None:
                    records.append((NULL, None))
                elif isinstance(v, _Ptr):
                    role = roles.get(i, IN)
                    records.append((role, v.array if role == OUT else v.array.copy()))
                else:
                    records.append((IN, _scalar(v)))
            ret = fn(*args)
            outputs = [v.array.copy() for i, v in enumerate(vals) if isinstance(v, _Ptr) and roles.get(i, IN) != IN]
            self._calls.append(Case(name, records, ret if name in RETURNS else None, outputs))
            return ret
        return call


@contextlib.contextmanager
def recording():
    """Within the block every orc_* call made through oracle.lib() is executed AND appended to the yielded list as a Case."""
    calls = []
    real_lib, real_p = oracle.lib, oracle._p
    rec = _Recorder(real_lib(), calls)

    def p(a, t=ctypes.c_void_p):
        ptr = _Ptr(a.ctypes.data)
        ptr.array = a
        return ptr
    oracle.lib, oracle._p = (lambda: rec), p
    try:
        yield calls
    finally:
        oracle.lib, oracle._p = real_lib, real_p


def write_case(path, case, fill, threads):
    with open(path, "wb") as f:
        f.write(struct.pack("<5I", 0x5243524F, FUNCS[case.name][0], fill, threads, len(case.records)))
        for role, a in case.records:
            if role == NULL:
                f.write(struct.pack("<3I", NULL, 0, 0))
                continue
            a = np.asarray(a)
            f.write(struct.pack("<3I", role, _CODE[a.dtype], a.ndim))
            f.write(struct.pack("<%dq" % a.ndim, *a.shape))
            if role != OUT:
                f.write(np.ascontiguousarray(a).tobytes())


def run(exe, case, fill=0, threads=1):
    """Replay `case` in the driver `exe` as a child process that cannot open a GPU. Returns (ret, outputs, report): ret and outputs
    as Case holds them (None when the driver failed), report = 'exit N: stderr' or '' for a clean run."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    with tempfile.TemporaryDirectory() as d:
        cpath, rpath = os.path.join(d, "case.bin"), os.path.join(d, "result.bin")
        write_case(cpath, case, fill, threads)
        pr = subprocess.run([exe, cpath, rpath], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL)
        report = "" if pr.returncode == 0 and not pr.stderr else "exit %d: %s" % (pr.returncode, pr.stderr.decode(errors="replace"))
        if pr.returncode != 0:
            return None, None, report
        with open(rpath, "rb") as f:
            raw = f.read()
    iret, fret = struct.unpack("<if", raw[:8])
    pos, outs = 8, []
    for role, a in case.records:
        if role in (OUT, INOUT):
            a = np.asarray(a)
            outs.append(np.frombuffer(raw, a.dtype, a.size, pos).reshape(a.shape).copy())
            pos += a.nbytes
    assert pos == len(raw), "result file has %d bytes, the case's outputs take %d" % (len(raw), pos)
    return (fret if case.name == "orc_resize_at" else iret), outs, report
