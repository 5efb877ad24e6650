"""Child process of test_sm4_wave_host_gpu.py: six 4-state reads, narrow (widest band at most 128 cells) and wide
(more than 128) in turn, through libcpecan_host.so under whatever CPECAN_SM4_WAVE the parent set -- the variable is
read by the library, so it has to be in the environment of a process of its own.  The reads go through one stream, the
chunk reports kept; `both`: also getAlignedPairsUsingAnchors on each read by itself.  Writes the triples of every read
and the chunks to the JSON file named first on the command line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "oracle")]
import stream_api as sa  # noqa: E402
from harness import cp  # noqa: E402

out, how = sys.argv[1], sys.argv[2]
JUMPS = [0, 110] * 3
sm, get_x = sa.machine("sm4")
reads = sa.synthetic_reads(45, [(360, 720)] * 6, get_x, jumps=JUMPS)
p = sa.params()
widths = [cp.band_extent(rd.anchors, rd.lX, rd.lY, 20)[0] for rd in reads]
assert all(w <= 128 for w in widths[0::2]) and all(w > 128 for w in widths[1::2]), widths
got = sa.run_stream(sm, reads, p, slots=2)
assert got["n_refused"] == 0 and sorted(got["delivered"]) == list(range(6))
result = dict(widths=widths, chunks=got["chunks"], reads=[got["results"][i].tolist() for i in range(6)])
if how == "both":
    result["alone"] = [sa.alone(sm, rd, p).tolist() for rd in reads]
json.dump(result, open(out, "w"))
