"""tools/msnv_mpileup checks its command line before it touches a device: usage without arguments, -B required, every samtools
option it does not build refused with exit status 1 and a message -- never ignored."""
import os
import subprocess

import pytest

from metasnv_amd import _lib

EXE = os.path.join(os.path.dirname(_lib.LIB_PATH), "tools", "msnv_mpileup")


def _run(*argv):
    return subprocess.run([EXE] + list(argv), capture_output=True, text=True, timeout=60)


def test_usage_without_arguments():
    r = _run()
    assert r.returncode == 1 and "Usage: msnv_mpileup" in r.stderr and r.stdout == ""


def test_baq_switch_is_required():
    r = _run("-f", "ref.fa", "-b", "list")
    assert r.returncode == 1 and "-B is required" in r.stderr and r.stdout == ""


@pytest.mark.parametrize("extra", [["-r", "c:1-5"], ["-E"], ["-u"], ["--rf", "2"], ["-Q", "x"], ["--ff", "zz"], ["--output-MQ"], ["extra.bam"]])
def test_other_samtools_options_are_refused(extra):
    r = _run("-f", "ref.fa", "-B", "-b", "list", *extra)
    assert r.returncode == 1 and r.stderr and r.stdout == ""
