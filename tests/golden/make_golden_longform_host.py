"""Generate tests/golden/longform_host.json: the case table of tests/longform_host_cases.py (scripted decoders, no
GPU) run on the long-form host logic of ONE commit, the one the refactor of the seek loop must reproduce.

    git worktree add --detach /tmp/parent <commit>
    python tests/golden/make_golden_longform_host.py --tree /tmp/parent

--tree: a checkout of that commit; its tw package is the one imported, the case table is this tree's.  Per case the
file holds the output ids, every _trace record without gate_ms, the decoder and keyword names of every run() call,
the shape of every encode() input, and whether the commit ran the case through its sequential loop (the one place
where tests/test_longform_host_cpu.py allows a difference: `batch`)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="checkout of the commit to record")
    tree = os.path.abspath(ap.parse_args().tree)
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(tree, "taiwan-whisper_amd"))
    from tw import generation
    assert os.path.abspath(generation.__file__).startswith(tree + os.sep), generation.__file__
    from longform_host_cases import CASES, run_case
    commit = subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], check=True, capture_output=True,
                            text=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", tree, "status", "--porcelain", "--untracked-files=no"], check=True,
                           capture_output=True, text=True).stdout.strip()
    assert not dirty, f"{tree} has local changes:\n{dirty}"
    cases = {}
    for name, case in CASES.items():
        cases[name] = dict(run_case(generation, case), sequential=case["sequential"])
    path = os.path.join(HERE, "longform_host.json")
    with open(path, "w") as f:
        json.dump(dict(commit=commit, cases=cases), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(cases)} cases from {commit}")


if __name__ == "__main__":
    main()
