#!/usr/bin/env python3
"""Writes tests/golden/launch/plans.json: the signatures (tests/launch_plans.py) of the launch lists of the Python-listed models.
Run from a checkout of the commit the plans are to be held to: `python tests/golden/launch/make_golden_launch.py COMMIT`
(COMMIT goes into the file as a note).  The stored file was recorded from 877fdad, the last commit on which every module kept a
list, a keep-alive list and a replay loop of its own."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))

from tests import launch_plans  # noqa: E402

if __name__ == "__main__":
    with open(os.path.join(HERE, "plans.json"), "w") as fh:
        plans = {k: v for build in launch_plans.BUILDERS.values() for k, v in build().items()}
        json.dump({"recorded_from": sys.argv[1], "plans": plans}, fh, separators=(",", ":"))
        fh.write("\n")
