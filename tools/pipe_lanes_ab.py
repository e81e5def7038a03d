"""bench.py with the sequence pipeline's chains / lanes choice forced (GPU box): the A/B rows of profiles/pipe_lanes.md.  bench.py
itself has no such switch and gets none: this script sets the defaults of FramePipeline's test keywords and runs bench.py unchanged
in the same process.
usage: python tools/pipe_lanes_ab.py <lanes: -1 auto | 0 chains | 1 lanes> <sets: 0 = default> <place: 0 | 1> [bench args...]"""
import functools
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orb_slam2_ssd_semantic_amd import pipeline  # noqa: E402

lanes, sets, place = (int(x) for x in sys.argv[1:4])
pipeline.FramePipeline.__init__ = functools.partialmethod(pipeline.FramePipeline.__init__, _lanes=lanes, _lane_sets=sets, _lane_place=place)
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[4:]
runpy.run_path(sys.argv[0], run_name="__main__")
