"""The dense-convolution routing of upsnet_amd.models.hipconv against a recorded table: for every layer geometry of the two presets, on
every map, flag, precision and knob of tests/conv_route_cases.py, the launcher called, every argument it got (split factor, n_main,
tile, dtypes after widening, which cached pack) and the trace records must equal tests/golden/conv_routes.json.gz, which was recorded
with the same recorder on the commit before the route / launch split. CPU only: the launchers are stubs on meta tensors."""
import fnmatch
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_route_cases as crc  # noqa: E402

# every form the table must reach at least once (fnmatch patterns; alternatives in one tuple)
NEED_FORMS = [('igemm',), ('igemm splitk*',), ('igemm multi',), ('igemm multi cat',), ('conv1x1',), ('conv1x1 main + tail splitk*', 'conv1x1 all splitk*'),
              ('conv1x1 ksw 16x64',), ('conv3x3 ksw 16x32',), ('winograd tm32',), ('winograd tm64',), ('winograd tm32 multi',), ('winograd tm64 multi',),
              ('winograd splitk*',), ('winograd tm32 + tail tn32',), ('winograd36',), ('winograd36 roi',), ('winograd36 multi',), ('winograd36 splitk*',),
              ('bf16 *',), ('bf16x3 *',), ('library',)]


@pytest.fixture(scope='module')
def golden():
    return crc.load()


def test_fixture_is_complete(golden):
    """The recorded table covers the grid of today, one record per case, and reaches every kernel form."""
    cases = [crc.case_id(c) for c in crc.grid()]
    assert len(golden['cases']) == len(golden['index']) == len(cases) and golden['cases'] == cases
    assert len(set(cases)) == len(cases)
    records = [golden['records'][i] for i in golden['index']]
    forms = crc.forms_of(records)
    for alternatives in NEED_FORMS:
        assert any(fnmatch.fnmatchcase(f, p) for f in forms for p in alternatives), (alternatives, forms)
    launches = [[e[0] for e in r['log'] if e[0] != 'cached_pack' and not e[0].startswith('pack_')] for r in records]
    tail = [names for r, names in zip(records, launches) if any(t[0] == 'winograd tm32 + tail tn32' for t in r.get('trace', ()))]
    assert ['conv2d_winograd_tail'] in tail and ['conv2d_winograd_multi', 'conv2d_winograd_multi'] in tail      # one launch and two
    raised = [r['raises'] for r in records if 'raises' in r]
    assert raised and set(raised) == {'RuntimeError'}        # only the layers hipconv.supported rejects, with the library not allowed
    assert len(raised) == sum(1 for c in crc.grid() if c[0] == 'fallback' and c[1] is False and c[5] == 'device')
    assert any(r.get('fallbacks') and any(t[0] == 'library' for t in r.get('trace', ())) for r in records)


def test_routes_equal_the_recorded_table(golden):
    cases, records = crc.record_all()
    bad = []
    for case, got, idx in zip(cases, records, golden['index']):
        want = golden['records'][idx]
        if json.loads(got) != want:
            bad.append(case)
            if len(bad) <= 10:
                print('%s\n  recorded: %s\n  now:      %s' % (crc.case_id(case), json.dumps(want, sort_keys=True), got))
    assert not bad, '%d of %d cases differ from the recorded table (first: %s)' % (len(bad), len(cases), crc.case_id(bad[0]))
