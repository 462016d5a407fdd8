"""Generate tests/golden/generate_host.json: the case table of tests/generate_plan_cases.py (scripted decoders, _detect
replaced, no GPU) run on generate's host side of ONE commit, the one a refactor of that host side must reproduce.

    git worktree add --detach /tmp/parent <commit>
    python tests/golden/make_golden_generate_host.py --tree /tmp/parent

--tree: a checkout of that commit; its tw package is the one imported, the case table is this tree's.  Per valid call
the file holds the form, every decoder built with its constructor arguments, the prompt rows and keyword names of
every run(), the (B, Tk) of every _detect call, the ids and the languages; per invalid call the exception type and
its message."""
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
    from generate_plan_cases import CASES, run_case
    commit = subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], check=True, capture_output=True,
                            text=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", tree, "status", "--porcelain", "--untracked-files=no"], check=True,
                           capture_output=True, text=True).stdout.strip()
    assert not dirty, f"{tree} has local changes:\n{dirty}"
    cases = {name: run_case(generation, case) for name, case in CASES.items()}
    path = os.path.join(HERE, "generate_host.json")
    with open(path, "w") as f:
        json.dump(dict(commit=commit, cases=cases), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(cases)} cases from {commit}")


if __name__ == "__main__":
    main()
