#!/usr/bin/env python3
"""Generates tests/golden/sw_edge_vectors.json from the REFERENCE's own Smith-Waterman objects
(oracle/_ref/libgkl_ref_sw.so, built by `make -C oracle ref`).  Run where the reference's sources are
present (`REF` of oracle/Makefile), like make_sw_fixtures.py:

    python tests/golden/make_sw_edge_fixtures.py

The cases are those of tests/sw_cases.py; the file holds RECIPES (family, ints, seed, params, strategy, cigar_len:
tests/sw_cases.expand() rebuilds the sequences) and the reference's answer for each: cigar text, cigar count, alignment
offset, identical for both engines (asserted here).  A subset of the whole set, chosen by sw_cases.fixture_subset so
that it still changes the answer of every one-comparison mutant of oracle/sw_oracle.c (asserted here and in
tests/test_sw_edges.py): it pins the oracle on machines without the reference."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.sw import SwOracle, SwReference  # noqa: E402
from tests import sw_cases  # noqa: E402


def main():
    ref, oracle = SwReference(), SwOracle()
    engines = (1, 2) if ref.has_avx512() else (1,)
    cases = sw_cases.all_cases()
    answers = [oracle.align(*sw_cases.expand(c), cigar_len=c.cigar_len) for c in cases]
    with tempfile.TemporaryDirectory() as d:
        counts = sw_cases.mutant_counts(cases, answers, sw_cases.build_mutants(d))
    keep = sw_cases.fixture_subset(cases, counts)
    for name, (_, _, hit, big) in counts.items():
        pool = big if name in sw_cases.MAXIMUM_MUTANTS else hit
        assert set(pool) & set(keep), name
    out = []
    for k in keep:
        c = cases[k]
        r, a, p, s = sw_cases.expand(c)
        res = [ref.align(r, a, p, s, cigar_len=c.cigar_len, engine=e) for e in engines]
        assert all(x == res[0] for x in res), c
        st, cig, cnt, off = res[0]
        assert st == 0
        v = sw_cases.case_to_json(c)
        v.update({"cigar": cig.decode("ascii"), "count": cnt, "offset": off})
        out.append(v)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sw_edge_vectors.json")
    with open(path, "w") as f:
        f.write('{"generator": "tests/golden/make_sw_edge_fixtures.py", "engines": %s, "vectors": [\n' % json.dumps(list(engines)))
        f.write(",\n".join(json.dumps(v, separators=(",", ":")) for v in out))
        f.write("\n]}\n")
    print(len(out), "vectors of", len(cases), "cases,", os.path.getsize(path), "bytes")
    for name, (n, nbig, _, _) in counts.items():
        print(f"{name}: {n} of {len(cases)} answers change, {nbig} with nrow + ncol > 128")


if __name__ == "__main__":
    main()
