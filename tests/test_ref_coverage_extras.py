"""tests/covextmodel.py against qaCompute.cpp itself, unchanged, built against htslib (oracle/_ref/qaCompute: `make -C oracle ref`):
`qaCompute -m -p W -x R -c N -d -i BAM OUT` on the BAMs of two record sets of tests/covmodel.py, four files each.  Skips where the
reference binary is not built, as tests/test_ref_builds.py does.

The model takes a contig on which a sample's depth is 0 everywhere through the no-reads path, the reference takes it through
compute_print_cov when mapped reads name it.  Every sample used here has a depth that is not zero on
every contig it has mapped reads on -- asserted below -- so the two agree on these inputs by construction."""
import os
import subprocess

import pytest

import bamtools as bt
import covmodel
import covextmodel as xm
import orc
from metasnv_amd import core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_QACOMPUTE = os.path.join(ROOT, "oracle", "_ref", "qaCompute")
need_qacompute = pytest.mark.skipif(not os.path.exists(REF_QACOMPUTE), reason="oracle/_ref/qaCompute not built (needs htslib: make -C oracle ref)")


@need_qacompute
@pytest.mark.parametrize("name,W", [("d_ends", 32), ("d_ends", 2048), ("f_copies", 33), ("f_copies", 5000)])
def test_extras_model_equals_the_reference_binary(name, W, tmp_path):
    case = covmodel.cases()[name]
    lines = [(case.names[-1], 0, 0, "first_index"), ("not_in_header", 1, 5, "outside"), (case.names[-1], 10, 2040, "span"),
             (case.names[0], 0, 0, "short_contig")]
    rfile = str(tmp_path / "regions.txt")
    with open(rfile, "w") as f:
        f.write("".join("%s\t%d\t%d\t%s\n" % ln for ln in lines))
    for s, records in enumerate(case.samples):
        dp = xm.sample_depths(case.lengths, records)
        mapped = {r["tid"] for r in bt.iter_records(records) if not (r["flag"] & 0x4) and r["tid"] >= 0}
        assert mapped == set(dp), "a contig with mapped reads and no depth: the documented divergence would show"
        bam, out = str(tmp_path / ("s%d.bam" % s)), str(tmp_path / ("s%d.cov" % s))
        core.write_bam(bam, case.names, case.lengths, records)
        r = subprocess.run([REF_QACOMPUTE, "-m", "-p", str(W), "-x", rfile, "-c", str(case.cov_max), "-d", "-i", bam, out], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        plain = orc.qacompute(case.names, case.lengths, records, max_cov=case.cov_max, min_mapq=1)
        assert open(out).read() == xm.cov_text_with_median(plain[0], len(case.names), xm.medians(case.lengths, dp))
        assert open(out + ".detail").read() == plain[1]
        assert open(out + ".profile").read() == xm.profile_text(case.names, case.lengths, dp, W)
        assert open(out + ".specific").read() == xm.specific_text(case.names, dp, lines)
