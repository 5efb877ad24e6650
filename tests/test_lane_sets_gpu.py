"""Lane sets (cpecan_hip.hip): a chain of batches runs on the three streams of the lane set its first batch ran on --
forward, back, post -- whatever the number of batches and contexts, so that it fits the four hardware queues a process
gets by default.  Each case runs in a fresh process with GPU_MAX_HW_QUEUES=4 (the runtime reads it once, at start) and
checks what the contract of cpecan_hip_batch_run_after promises (include/cpecan_hip.h): results bit-identical to the
oracle, a batch read back through its own end event while a follower is still queued on the same lanes, a leader's
context destroyed under a running follower, model tables rebuilt on a context whose batch ran on another context's
lanes, and runs issued from two host threads onto one lane set.

Reads shaped for the assembly sweeps, as in test_chained_batches_gpu.py: 8 reads of about 1 200 k-mers x 2 400 events,
diagonalExpansion 100, a traceback every 300 diagonals: 8 and more windows."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 8
_DATA = {}
_ORACLE = {}


def _setup():
    try:  # the first HIP runtime loaded in the process (see conftest.py)
        import torch  # noqa: F401
    except ImportError:
        pass
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _h():
    import harness
    return harness


def asm_bp():
    return _h().band_params(0.01, 300, 40, 100)


def data(seed):
    import pyoracle as o
    import synth
    if seed not in _DATA:
        bt = synth.make_batch(seed, N, 1200, 2400, anchor_every=50, length_sigma=0.2)
        match, gx, gy = bt["base_model"]
        base = o.Sm3Model(match, gy, gx)
        bt["models"] = [(base.scaled(*[float(v) for v in sc]).match, gx, gy) for sc in bt["scalings"]]
        _DATA[seed] = bt
    return _DATA[seed]


def new_batch(cx, seed, model_base=0, clear=True):
    h = _h()
    cp, bt = h.cp, data(seed)
    if clear:
        cx.models_clear()
    cx.models_create_scaled((cp.NANOPORE_TRANSITIONS,) + bt["base_model"], bt["scalings"])
    items = h.make_items(bt, (1, 1))
    items["model_id"] += model_base
    b = cp.Batch(cx, items, bt["x_chars"], bt["events"], bt["anchors"], asm_bp(), cp.MODE_POSTERIOR, cp.KERNEL_AUTO, 0)
    info = b.info()
    assert info["assembly_sweeps"] == 2 and 121 <= info["max_band_width"] <= 158, info
    b.seed = seed
    return b


def check(b):
    """the batch's results through its own readback, against the oracle"""
    h = _h()
    for i, g in enumerate(h.batch_results(b)):
        key = (b.seed, i)
        if key not in _ORACLE:
            _ORACLE[key] = h.run_oracle_item(data(b.seed), i, asm_bp(), (1, 1))
        h.assert_same_posterior(g, _ORACLE[key], key)


def results(b):
    """every array the readback gives, for comparisons between runs"""
    return [{k: getattr(v, "copy", lambda: v)() for k, v in r.items()} for r in _h().batch_results(b)]


def same(ra, rb):
    import numpy as np
    assert len(ra) == len(rb)
    for x, y in zip(ra, rb):
        assert sorted(x) == sorted(y)
        for k in x:
            assert np.array_equal(x[k], y[k], equal_nan=True), k


# ---- the cases, each in a child process (python tests/test_lane_sets_gpu.py CASE) ----

def case_ping_pong():
    """bench.py's schedule for five rounds: step s on batch s % 2 behind step s - 1's batch, a batch waited for only
    when it is needed again, and compared with the oracle after every wait"""
    cp = _h().cp
    ctxs = [cp.Context(0) for _ in range(2)]
    bs = [new_batch(cx, 301 + k) for k, cx in enumerate(ctxs)]
    pending = [False, False]
    for s in range(10):
        j = s % 2
        if pending[j]:
            bs[j].sync()
            check(bs[j])
        bs[j].run(after=bs[(s - 1) % 2] if s > 0 else None)
        pending[j] = True
    for k in range(2):
        bs[k].sync()
        check(bs[k])
    for cx in ctxs:
        cx.close()


def case_leader_read_while_follower_queued():
    """the leader synced and read back on its own while two followers are queued behind it on the same lanes"""
    cp = _h().cp
    ctxs = [cp.Context(0) for _ in range(3)]
    a, b, c = (new_batch(cx, 311 + k) for k, cx in enumerate(ctxs))
    a.run()
    b.run(after=a)
    c.run(after=b)
    a.sync()
    check(a)
    c.sync()
    check(b)
    check(c)
    for cx in ctxs:
        cx.close()


def case_leader_context_destroyed():
    """the leader's context (its lanes' owner) destroyed while the follower runs on those lanes; the follower then runs
    again on its own context's lanes"""
    cp = _h().cp
    c0, c1 = cp.Context(0), cp.Context(0)
    a = new_batch(c0, 321)
    b = new_batch(c1, 322)
    a.run()
    b.run(after=a)
    c0.close()  # closes a (waits for its run), then the context: the lanes stay while b holds them
    b.sync()
    check(b)
    b.run()
    b.sync()
    check(b)
    c1.close()


def case_models_rebuilt():
    """models added to, and cleared on, a context whose last batch ran on another context's lanes: the fence waits for
    that batch's run wherever it went, and nothing it read is released under it"""
    cp = _h().cp
    c0, c1 = cp.Context(0), cp.Context(0)
    a = new_batch(c0, 331)
    b = new_batch(c1, 332)
    a.run()
    b.run(after=a)
    b2 = new_batch(c1, 333, model_base=N, clear=False)  # grows c1's table while b may still be sweeping
    b2.run(after=b)
    c1.models_clear()  # releases c1's tables: b and b2 must be over
    # other tables at once, into the blocks just released: a run still reading c1's old tables would read these
    bt = data(334)
    c1.models_create_scaled((cp.NANOPORE_TRANSITIONS,) + bt["base_model"], bt["scalings"])
    check(a)
    check(b)
    check(b2)
    b.close()
    b2.close()
    b3 = new_batch(c1, 334)
    b3.run(after=a)
    b3.sync()
    check(b3)
    c0.close()
    c1.close()


def case_transitions_rewritten_under_queued_follower():
    """the transitions of a context rewritten in place (cpecan_hip_models_set_transitions) right after its batch was
    queued behind another context's batch, on that batch's lanes: the rewrite waits for the run, which must see the
    transitions it was queued with"""
    cp = _h().cp
    c0, c1 = cp.Context(0), cp.Context(0)
    a = new_batch(c0, 351)
    b = new_batch(c1, 352)
    a.run()
    b.run(after=a)  # queued behind a's forward sweeps: it has not started yet
    t = list(cp.NANOPORE_TRANSITIONS)
    t[0] -= 0.05  # (the gap switches stay -inf: the run's kernels were chosen for that)
    t[3] += 0.05
    c1.models_set_transitions(t)
    check(a)
    check(b)
    c0.close()
    c1.close()


def case_refused_batches_leave_the_context_whole():
    """batches refused at creation (a band too wide for the systolic kernels, cell dumps from them) are taken off the
    context's list: the fences of later model calls and of the context's destruction see only live batches"""
    import synth
    h = _h()
    cp = h.cp
    cx = cp.Context(0)
    wide = (synth.make_batch(24, 1, 400, 800, anchor_every=400), h.band_params(0.01, 200, 40, 300), 0)  # band > 256
    dump = (synth.make_batch(25, 2, 150, 310, anchor_every=25), h.band_params(0.01, 80, 20, 40), cp.FLAG_DEBUG_DUMP)
    for _ in range(3):
        for batch, bp, flags in (wide, dump):
            try:
                h.run_gpu(cx, batch, bp, kernel=cp.KERNEL_SYSTOLIC, flags=flags)
            except cp.CpecanError as e:
                assert e.code == cp.EINVAL
            else:
                raise AssertionError("the systolic kernels took a batch they must refuse")
    b = new_batch(cx, 361)  # models cleared and created (fenced), then a batch that runs
    b.run()
    b.sync()
    check(b)
    cx.models_set_transitions(cp.NANOPORE_TRANSITIONS)
    cx.close()


def case_two_threads():
    """two host threads, each with a context of its own, each issuing runs behind a leader of a third context (onto
    that leader's lanes) and unchained runs (on its own lanes): every result identical to a serial run's"""
    import threading
    cp = _h().cp
    c0 = cp.Context(0)
    lead = new_batch(c0, 341)
    lead.run()
    lead.sync()
    check(lead)
    ctxs = [cp.Context(0) for _ in range(2)]
    mine = [[new_batch(cx, 342 + 2 * t), new_batch(cx, 343 + 2 * t, model_base=N, clear=False)]
            for t, cx in enumerate(ctxs)]
    serial = []
    for t in range(2):
        for b in mine[t]:
            b.run()
            b.sync()
            check(b)
        serial.append([results(b) for b in mine[t]])
    errors = []

    def work(t):
        try:
            x, y = mine[t]
            for r in range(4):
                x.run(after=lead)  # on c0's lanes, as the other thread's runs are
                if r % 2:
                    y.run()
                else:
                    y.run(after=x)  # behind this thread's own run on c0's lanes
                y.sync()
                x.sync()
                same(results(x), serial[t][0])
                same(results(y), serial[t][1])
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if errors:
        raise errors[0]
    for cx in ctxs + [c0]:
        cx.close()


CASES = {k[5:]: v for k, v in dict(globals()).items() if k.startswith("case_")}


@pytest.mark.parametrize("name", sorted(CASES))
def test_lane_sets(name):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=env, cwd=ROOT, timeout=900,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "case ok" in r.stdout, r.stdout[-4000:]


if __name__ == "__main__":
    _setup()
    CASES[sys.argv[1]]()
    print("case ok:", sys.argv[1])
