"""CPU check of the main library's host rules (snappy.jl_amd/csrc/sm_host_rules.h, sm_format.h):
the stand-alone sanitizer driver.  No kernel is launched here."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "snappy.jl_amd", "csrc")


def test_host_check_runs_clean(tmp_path):
    """make host_check: literal_only, host_walk, the true path and its fragment table, the shards,
    the length check, the varint header and every scratch layout of sm_api.hip against the oracle
    and a walker of the driver's own, under ASan and UBSan, as a stand-alone program."""
    r = subprocess.run(["make", "-C", CSRC, "host_check", "OBJ=%s" % tmp_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sm_host_check: ok" in r.stdout
