"""Outcome table of the argument-form sweep (tests/test_abi_contract_gpu.py) for two trees side by side.

The sweep writes one JSON row per (entry point, argument, variant) when UPSNET_ABI_FORMS_JSON names a file:

    UPSNET_ABI_FORMS_JSON=parent.jsonl python -m pytest -m gpu tests/test_abi_contract_gpu.py -k test_every_argument_form   # in the parent tree
    UPSNET_ABI_FORMS_JSON=new.jsonl    python -m pytest -m gpu tests/test_abi_contract_gpu.py -k test_every_argument_form   # in this tree
    python tools/abi_forms.py parent.jsonl new.jsonl > profiles/abi_forms.txt

The guard and the sweep are test-side, so the same test files run against either tree's package (the `offset` rows of a parent from
before the alignment rule are made that way: this tree's tests/ over the parent's upsnet_amd/). Exit status 1 if a row goes from
`same` to `refused`, or is neither `same` nor `refused` in the new column.
"""
import collections
import json
import re
import sys


def load(path):
    rows = collections.OrderedDict()
    with open(path) as f:
        for line in f:
            if line.strip():
                entry, arg, variant, outcome, detail = json.loads(line)
                rows[(entry, arg, variant)] = (outcome, detail)
    return rows


def short(outcome, detail):
    if outcome == 'violation':
        m = re.search(r': (origin|liveness|element type|density|device|alignment): ', detail)
        return 'VIOLATION (%s)' % (m.group(1) if m else '?')
    return outcome if outcome in ('same', 'refused') else outcome.upper()


def main(parent_path, new_path):
    parent, new = load(parent_path), load(new_path)
    keys = list(new) + [k for k in parent if k not in new]
    findings = [k for k in parent if parent[k][0] not in ('same', 'refused')]
    tightened = [k for k in keys if k in parent and k in new and parent[k][0] == 'same' and new[k][0] == 'refused']
    open_rows = [k for k in new if new[k][0] not in ('same', 'refused')]
    count = lambda rows: dict(collections.Counter(short(*v).split(' ')[0] for v in rows.values()))     # noqa: E731
    print("# Argument forms across the C ABI: tests/test_abi_contract_gpu.py, form sweep, parent tree and this tree (tools/abi_forms.py)")
    print("# rows: %d (parent %d)   parent: %s   new: %s" % (len(new), len(parent), count(parent), count(new)))
    print("# findings (rows that are neither same nor refused at the parent): %d" % len(findings))
    for v in sorted({k[2] for k in keys}, key=[k[2] for k in keys].index):
        print("#   %-14s parent: %s   new: %s" % (v, count({k: r for k, r in parent.items() if k[2] == v}), count({k: r for k, r in new.items() if k[2] == v})))
    print("# same -> refused: %d   neither same nor refused in the new column: %d" % (len(tightened), len(open_rows)))
    print("# refused: ValueError / TypeError / RuntimeError from the wrapper before any entry point that takes a pointer was called (size")
    print("#   queries such as upsnet_*_workspace_bytes take none and launch nothing: they do not count)")
    print("# VIOLATION (rule): tests/abiguard.py refused the call before the library was entered, so what the kernel would have made of")
    print("#   it was not observed; RAISED ASSERTIONERROR: the wrapper's own `assert`, which python -O removes; '(as the case calls it)':")
    print("#   the case's own call breaks a rule, no variant was tried; '-': no such row in that tree")
    w = [max(len(k[i]) for k in keys) for i in range(3)]
    print("%-*s  %-*s  %-*s  %-26s %s" % (w[0], 'entry point', w[1], 'argument', w[2], 'variant', 'parent', 'new'))
    for k in keys:
        p = short(*parent[k]) if k in parent else '-'
        n = short(*new[k]) if k in new else '-'
        print("%-*s  %-*s  %-*s  %-26s %s" % (w[0], k[0], w[1], k[1], w[2], k[2], p, n))
    return 1 if tightened or open_rows else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
