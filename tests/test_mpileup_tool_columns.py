"""tools/msnv_mpileup takes -a, -aa, -a -a, -s, -O and --output-BP (msnv_mpileup_text_opts): each gets past the option parsing, which
is seen without a device from the first thing the tool does behind it -- it opens the BAM list."""
import os
import subprocess

import pytest

from metasnv_amd import _lib

EXE = os.path.join(os.path.dirname(_lib.LIB_PATH), "tools", "msnv_mpileup")


@pytest.mark.parametrize("extra", [["-a"], ["-aa"], ["-a", "-a"], ["-s"], ["-O"], ["--output-BP"], ["-aa", "-s", "-O"], ["-asO"]])
def test_the_column_options_get_past_option_parsing(extra, tmp_path):
    missing = str(tmp_path / "no_such_list")
    r = subprocess.run([EXE, "-f", "ref.fa", "-B", "-b", missing] + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    assert "cannot open" in r.stderr and "not supported" not in r.stderr


def test_usage_names_the_options_and_the_spelling_of_mapq_output():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    for word in ("-aa", "-s", "--output-BP", "--output-MQ"):
        assert word in r.stderr
