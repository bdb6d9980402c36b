"""Recorded outputs of the reference's own binaries -- TEST INFRASTRUCTURE ONLY.

The reference's kernels (hipified into oracle/_ref/ by `make -C oracle ref`) and its Cython cpu_nms module can only be built
where the reference tree is present. The tests that pin the oracle and the HIP kernels against them (tests/test_ref_cpu_nms.py,
tests/test_ref_kernels_gpu.py, tests/test_backward_gpu.py) therefore replay what those binaries returned, recorded once into
tests/golden/ref_*.npz by running the same tests with the binaries present:

    REFVEC_RECORD=1 python -m pytest tests/test_ref_cpu_nms.py
    REFVEC_RECORD=1 python -m pytest tests/test_ref_kernels_gpu.py tests/test_backward_gpu.py      (on the GPU)

A call is looked up by a digest of its name and of all its inputs: a test whose inputs change finds no record and fails. To stay
small a record holds the difference between the reference's output and the oracle's result for the same call (nothing where
they agree bit for bit), plus the sha256 of the reference's exact output, which every replayed output is checked against.
"""
import ctypes
import hashlib
import os

import numpy as np

RECORD = os.environ.get('REFVEC_RECORD', '0') == '1'


def _update(h, a):
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a)
        h.update(('%s%s' % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    else:
        h.update(repr(a).encode())     # (float repr round-trips)
    h.update(b'|')


def digest(a):
    h = hashlib.sha256()
    _update(h, np.asarray(a))
    return h.hexdigest()


class RefVectors(object):
    """The recorded outputs of one test module, stored in `path` (.npz)."""

    def __init__(self, path):
        self.path = path
        self.new = {}
        self._data = None

    def _records(self):
        if self._data is None:
            if not os.path.exists(self.path):
                raise FileNotFoundError('%s missing: record it (oracle/refvec.py)' % self.path)
            with np.load(self.path) as z:
                self._data = {k: z[k] for k in z.files if not k.startswith('_')}
                for k, h, t in zip(z['_keys'], z['_sha'].astype(str), z['_dtype'].astype(str)):
                    self._data[k + '.sha'], self._data[k + '.dtype'] = h, t
        return self._data

    def __call__(self, name, args, oracle_out, run):
        """The reference's output of call `name` on inputs `args`: run() in record mode, else the record. oracle_out: the oracle's
        result for the same call (an array, a tuple of arrays like run()'s, or None); the record is stored relative to it."""
        h = hashlib.sha1(name.encode())
        for a in args:
            _update(h, a)
        key = '%s.%s' % (name, h.hexdigest()[:16])
        if RECORD:
            out = run()
            parts = out if isinstance(out, tuple) else (out,)
            bases = oracle_out if isinstance(oracle_out, tuple) else (oracle_out,) * len(parts)
            for i, (o, b) in enumerate(zip(parts, bases)):
                self._store('%s.%d' % (key, i), np.asarray(o), b)
            return out
        rec = self._records()
        if key + '.0.sha' not in rec:
            raise KeyError('no recorded reference output for %s with these inputs in %s: re-record it (oracle/refvec.py)' % (name, self.path))
        n = sum(1 for k in rec if k.startswith(key + '.') and k.endswith('.sha'))
        bases = oracle_out if isinstance(oracle_out, tuple) else (oracle_out,) * n
        parts = tuple(self._load(rec, '%s.%d' % (key, i), bases[i], name) for i in range(n))
        return parts if n > 1 else parts[0]

    def _store(self, k, out, base):
        self.new[k + '.sha'], self.new[k + '.dtype'] = digest(out), out.dtype.str
        if base is not None and np.shape(base) == out.shape and out.dtype.kind in 'fiu':
            b = np.asarray(base).astype(out.dtype)
            if b.tobytes() == out.tobytes():
                return
            d = out - b
            if (b + d).tobytes() == out.tobytes():
                self.new[k + '.d'] = d
                return
        self.new[k + '.out'] = out

    def _load(self, rec, k, base, name):
        if k + '.out' in rec:
            out = rec[k + '.out']
        elif k + '.d' in rec:
            d = rec[k + '.d']
            out = np.asarray(base).astype(d.dtype) + d
        else:                          # bit-equal to the oracle's result
            out = np.asarray(base).astype(rec[k + '.dtype'])
        assert digest(out) == rec[k + '.sha'], \
            'the record of %s no longer reproduces the reference output (did the oracle change?): re-record it' % name
        return out

    def save(self):
        """Record mode: merge the outputs recorded by this run into the .npz."""
        if not RECORD or not self.new:
            return
        rec = dict(self._records()) if os.path.exists(self.path) else {}
        rec.update(self.new)
        keys = sorted(k[:-4] for k in rec if k.endswith('.sha'))
        arrays = {k: v for k, v in rec.items() if not k.endswith(('.sha', '.dtype'))}
        np.savez_compressed(self.path, _keys=np.array(keys), _sha=np.array([rec[k + '.sha'] for k in keys], 'S64'),
                            _dtype=np.array([rec[k + '.dtype'] for k in keys], 'S8'), **arrays)
        self.new, self._data = {}, None


class RefLib(object):
    """One of the reference's kernel libraries in oracle/_ref/: loaded in record mode only; calls go through `vectors`."""

    def __init__(self, vectors, path):
        self.vectors, self.name = vectors, os.path.splitext(os.path.basename(path))[0]
        self.lib = None
        if RECORD:
            assert os.path.exists(path), "%s missing: run `make -C oracle ref` where the reference tree exists" % path
            self.lib = ctypes.CDLL(path)

    def __call__(self, fn, args, oracle_out, run):
        """run(lib) -> the output of the reference's `fn` on `args` (numpy arrays)."""
        return self.vectors('%s.%s' % (self.name, fn), args, oracle_out, lambda: run(self.lib))
