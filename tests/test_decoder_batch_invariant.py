"""The invariant behind the decoder's once-per-batch checks (no GPU): compiled with gcc and run.

tools/check_tag_lengths.c goes through every (tag byte, next byte) and checks that a tag whose
speculative size is not 255 -- the only kind the window walk hands to a lane -- is a copy of at
most 64 bytes or a literal of at most 200, with the size the clean-batch lemma relies on."""
import os
import re
import subprocess

from conftest import ROOT


def test_walked_tags_have_bounded_lengths(tmp_path):
    exe = tmp_path / "check_tag_lengths"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tools", "check_tag_lengths.c")],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    m = re.match(r"bad 0 of (\d+) walked tags, longest copy (\d+), longest literal (\d+)", out)
    assert m, out
    assert int(m.group(1)) > 200 * 256 * 5 and int(m.group(2)) == 64 and int(m.group(3)) == 200, out
