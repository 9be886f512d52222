"""profiles/multi_build_counts.py -- the static instruction counts of accumulate_multi_kernel's build phase -- runs on the tree, and
the counts committed as profiles/multi_build_counts.json are those of the tree's own kernel text (a change of kiwi_accum.inc that
moves them has to commit them again).  Needs the compiler, no GPU."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc: the counts come from the compiler's assembly")
def test_committed_counts_are_the_trees(tmp_path):
    out = tmp_path / "counts.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "multi_build_counts.py"), "--json", str(out)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    fresh = json.load(open(out))
    committed = json.load(open(os.path.join(ROOT, "profiles", "multi_build_counts.json")))
    assert [(k["kernel"], k["arith"]) for k in fresh] == [(k, a) for a in ("exact", "fused")
                                                          for k in ("accumulate_multi_kernel<10, true, 4, true, true>",
                                                                    "accumulate_multi_kernel<10, true, 2, true, true>")]
    for k in fresh:
        segs = k["raise_to_drop"]["segments"]
        assert k["priority_raises"] == k["priority_drops"] == 1 and k["spilled_sgprs"] >= 0
        assert k["raise_to_drop"]["total"]["packed"] > 0 and k["raise_to_drop"]["total"]["barrier"] == len(segs) - 1
        assert sum(s["all"] for s in segs) == k["raise_to_drop"]["total"]["all"] <= k["whole_kernel"]["all"]
    ver = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--version"], capture_output=True, text=True).stdout.strip().split("\n")
    assert fresh == committed, ("the kernel text's counts are not the committed ones.  If kiwi_accum.inc changed, or the compiler schedules "
                                "differently (the counts are one compiler's: %s), regenerate both records with that compiler -- "
                                "`python profiles/multi_build_counts.py --json profiles/multi_build_counts.json` on the tree and the "
                                "same on a checkout of the parent commit for multi_build_counts_parent.json -- and commit them"
                                % (ver[0] if ver else "version unknown"))
    # the parent's counts stay on record next to them: same kernels, same classes
    parent = json.load(open(os.path.join(ROOT, "profiles", "multi_build_counts_parent.json")))
    assert [(k["kernel"], k["arith"]) for k in parent] == [(k["kernel"], k["arith"]) for k in committed]
