#!/usr/bin/env python3
"""Writes tests/golden/launch/plans.json: the signatures (tests/launch_plans.py) of the launch lists of the Python-listed models.
Run from a checkout of the commit the plans are to be held to: `python tests/golden/launch/make_golden_launch.py COMMIT`
(COMMIT goes into the file as a note).  With `--add` behind COMMIT the keys that plans.json already holds stay as they are and
only the missing ones are recorded, with a note of their own.  The stored file was recorded from 877fdad, the last commit on
which every module kept a list, a keep-alive list and a replay loop of its own; the weight tables (``*.wtab``), the detector's pack
offsets (``*.layout``) and the f16 detector (``d0.f16.*``) were added from ddc7f86, the last commit on which every planner built
them for itself.

With `--detector-train` behind COMMIT it writes detector_train.json instead and leaves plans.json alone: the detector's training
lists at every depth (launch_plans.DETECTOR_TRAIN), each with its signature and its aliasing record.  The stored file was recorded
with stlpose_amd/ as of a609416, the last commit on which one class listed every training stage in three methods."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))

from tests import launch_plans  # noqa: E402


def dump(doc, name):
    with open(os.path.join(HERE, name), "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    if sys.argv[2:] == ["--detector-train"]:
        dump({"recorded_from": sys.argv[1], "plans": {k: launch_plans.detector_train(k) for k in launch_plans.DETECTOR_TRAIN}},
             "detector_train.json")
        sys.exit(0)
    path = os.path.join(HERE, "plans.json")
    plans = {k: v for build in launch_plans.BUILDERS.values() for k, v in build().items()}
    doc = {"recorded_from": sys.argv[1], "plans": plans}
    if sys.argv[2:] == ["--add"]:
        doc = json.load(open(path))
        new = {k: v for k, v in plans.items() if k not in doc["plans"]}
        doc["plans"].update(new)
        doc.setdefault("added", {})[sys.argv[1]] = sorted(new)
    dump(doc, "plans.json")
