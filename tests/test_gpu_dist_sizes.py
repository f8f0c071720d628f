"""metaSNV_DistDiv.py --dist on the device at the sizes real *.filtered.freq tables have: more than 8192 positions (numpy
sums in 8192-element blocks), more leaf sums than msnv_dist_pairs keeps in LDS (global scratch), up to 70 samples.
Byte-identical with what the reference wrote for the long tables of tests/golden/python_callers/dist_long (regenerated
here from their seeds, never stored) and with the numpy model tests/distmodel.py, which tests/test_dist_model.py pins
without a device.  Every comparison is string equality."""
import os
import shutil

import pytest

import distmodel
from distmodel import LONG, long_cases, long_table

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", LONG)
def test_long_tables_match_the_reference_files(tmp_path, golden_dir, case):
    """Through the driver (distdiv.main), --matched included: the reference's --dist does not filter the rows, it only writes
    into distances<pars>.matched_pos."""
    from metasnv_amd import distdiv
    spec = long_cases(golden_dir)[case]
    names, text, want = long_table(golden_dir, case)
    proj = str(tmp_path / "proj")
    pop = distmodel.write_project(proj, case, text)
    distdiv.main(["--filt", pop] + spec["options"])
    assert [d for d in os.listdir(proj) if d.startswith("distances")] == [spec["outdir"]]
    out = os.path.join(proj, spec["outdir"])
    assert sorted(os.listdir(out)) == sorted(want)
    wrong = distmodel.cells_differing(open(os.path.join(out, case + ".filtered.mann.dist")).read(), want[case + ".filtered.mann.dist"])
    print(case, "cells of .mann.dist that differ from the reference:", wrong)
    for f in sorted(want):
        assert open(os.path.join(out, f)).read() == want[f], (case, f)


def test_sweep_of_lengths_and_widths_against_the_model(tmp_path):
    """distmodel.sweep(): n_pos 0 (header only) to 65545 around the leaf and block boundaries, the lengths on both sides of the
    LDS / scratch crossover, 1 to 65 samples.  Before a table longer than 8192 rows with at least 6 pairs counts, the model
    itself must print it differently under the flat plan -- a condition on the inputs (distmodel.must_differ), so that a
    kernel that summed one flat tree could not pass."""
    import ctypes as C
    from metasnv_amd import core, _lib
    ctx = core.Context(0)
    guarded = routes = 0
    try:
        for seed, n_pos, S in distmodel.sweep():
            names, text = distmodel.make_table(seed, n_pos, S)
            path = str(tmp_path / "t.filtered.freq")
            with open(path, "w") as f:
                f.write(text)
            _, values = distmodel.read_table(text)
            assert values.shape == (n_pos, S)
            want = distmodel.dist_texts(names, values)
            if distmodel.must_differ(n_pos, S):
                flat = distmodel.dist_texts(names, values, plan=distmodel.flat_sum)
                assert distmodel.cells_differing(flat[0], want[0]) >= 1, (seed, n_pos, S)
                guarded += 1
            routes |= 2 if distmodel.n_leaves(n_pos) > distmodel.MAX_LEAVES_LDS else 1
            ns, npos = C.c_int32(), C.c_uint64()
            _lib.check(_lib.lib.msnv_dist_file(ctx._h, path.encode(), (path + ".mann").encode(), (path + ".allele").encode(), 0.6,
                                               C.byref(ns), C.byref(npos), None))
            assert (ns.value, npos.value) == (S, n_pos)
            got = open(path + ".mann").read(), open(path + ".allele").read()
            print(seed, n_pos, S, "mann cells differing:", distmodel.cells_differing(got[0], want[0]) if got[0].count("\n") == S + 1 else "shape")
            assert got[0] == want[0], (seed, n_pos, S)
            assert got[1] == want[1], (seed, n_pos, S)
    finally:
        ctx.close()
    assert guarded == 7 and routes == 3
