"""Reads whose alignment path runs at a chosen place in the band: on its lower edge (the cell of least x on each
diagonal, xmin), on its upper edge (xmax), a given number of cells inside or outside either, or across it.

synth.make_read puts the anchors on the true path, so the band is centred on the path and its edge cells hold almost no
mass: a kernel that gets an edge cell wrong leaves every total and pair unchanged.  Here the order is the other way
round: the anchors come first (on a nominal path drawn like make_read's), the band follows from them (o.band), and only
then is the read's own event-to-k-mer path drawn, one step at a time, to stay at the prescribed offset from the chosen
edge; the events are emitted from that path as make_read emits them.  Posteriors of such reads are as sharp as those of
make_read's, so the mass follows the path onto the edge.

Coordinates are the band's: cell (x, y) has consumed x k-mers and y events, diagonal d = x + y, xmy = x - y, and
diagonal d holds the cells L[d] <= xmy <= R[d] (steps of two).  A match step goes (x, y) -> (x + 1, y + 1) and emits
event y from k-mer x; a gap-Y step (a stay) goes to (x, y + 1) and emits event y from k-mer x - 1; a gap-X step (a
skipped k-mer) goes to (x + 1, y) and emits nothing.
"""
import numpy as np

import pyoracle as o
import synth

# the widest band each build takes (k-mers): the workgroup family's waves, the wave family's cells per lane, the
# assembly sweeps (three cells per lane, 121..158)
WG1, WAVE_L2, ASM_MAX, WAVE_L3, WAVE_L4 = 56, 120, 158, 184, 248
MAX_STAYS = 8
HDP_SD = 1.0


def nominal_counts(rng, lX, lY, skip=None):
    """events per k-mer as make_read draws them (0 with p = .1, else 1 + geometric stays, forced to sum to lY).
    skip = (a, S, dwell): k-mers a .. a + S - 1 emit nothing and k-mer a - 1 emits `dwell` events, the others at least
    one each"""
    stay = max(0.05, min(0.9, 1.0 - 0.9 * lX / max(lY, 1))) if lY > 0.9 * lX else 0.05
    counts = np.where(rng.random(lX) < 0.10, 0, rng.geometric(1.0 - stay, lX))
    fixed = np.zeros(lX, bool)
    if skip is not None:
        a, S, dwell = skip
        counts[a:a + S] = 0
        counts[a - 1] = dwell
        fixed[a - 1:a + S] = True
        free = ~fixed
        counts[free] = np.maximum(counts[free], 1)
    diff = int(lY - counts.sum())
    while diff != 0:
        if diff > 0:
            pick = rng.choice(np.flatnonzero(~fixed), size=diff)
            np.add.at(counts, pick, 1)
        else:
            nz = np.flatnonzero((counts > (1 if skip is not None else 0)) & ~fixed)
            pick = rng.choice(nz, size=min(-diff, nz.size), replace=False)
            counts[pick] -= 1
        diff = int(lY - counts.sum())
    return counts


def anchors_of(counts, every, skip=None):
    """every `every`-th k-mer that emitted, at its first event (make_read's rule without the jitter); none inside a
    skipped stretch, so that one anchor pair spans it"""
    lX = len(counts)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    out = []
    px = py = -1
    for x0 in range(every // 2, lX, every):
        x = x0
        while x < lX and counts[x] == 0:
            x += 1
        if x >= lX:
            break
        if skip is not None and skip[0] - 1 < x0 < skip[0] + skip[1]:
            continue
        if x > px and first[x] > py:
            out.append((x, int(first[x])))
            px, py = x, int(first[x])
    if skip is not None:  # the stretch's two ends: its dwell k-mer and the first k-mer after it
        a, S, _ = skip
        out = [p for p in out if not a - 1 <= p[0] <= a + S] + [(a - 1, int(first[a - 1])),
                                                                              (a + S, int(first[a + S]))]
        out.sort()
    return np.array(out, np.int64).reshape(-1, 2)


def widest(anchors, lX, lY, e):
    L, R = o.band(anchors, lX, lY, e)
    return int(((R - L) // 2 + 1).max())


def target_of(L, R, place, offset, cross=None):
    """the wanted xmy on every diagonal: `offset` cells inside the lower (place 'lower') or upper edge (negative: that
    many cells outside it); cross = (d0, d1): lower edge up to d0, upper edge from d1, a straight line between"""
    lo = L + 2 * offset
    hi = R - 2 * offset
    if place == "lower":
        return lo
    if place == "upper":
        return hi
    d0, d1 = cross
    d = np.arange(len(L))
    f = np.clip((d - d0) / max(d1 - d0, 1), 0.0, 1.0)
    t = np.rint((1 - f) * lo + f * hi).astype(np.int64)
    return t + ((t + d) & 1)  # xmy has the parity of its diagonal


def walk(rng, lX, lY, target):
    """the path from (0, 0) to (lX, lY) whose xmy stays as close to target[d] as the steps allow: a match step
    wherever it is as close as a gap step, else the closer gap step.  The strawMan machine has no gap X <-> gap Y
    switch, so a match step comes between a skip and a stay; no k-mer gets more than MAX_STAYS stays (where the edge
    runs along one k-mer for longer, at the read's first k-mer say, the path leaves it for a while), and no stay comes
    before the first k-mer (the model emits it from no k-mer).  Returns (the k-mer of every event (len lY), the path's
    cells (x, y) in order, (0, 0) first)."""
    x = y = run = 0
    last = "M"
    ev_kmer = []
    cells = [(0, 0)]
    while x < lX or y < lY:
        opts = []
        if x < lX and y < lY:
            opts.append((abs(x - y - target[x + y + 2]), 0 if run < MAX_STAYS else -1, "M"))
        if x < lX and (last != "Y" or y == lY):
            opts.append((abs(x + 1 - y - target[x + y + 1]), 1 + rng.random(), "X"))
        if y < lY and (x > 0 or x == lX) and (last != "X" or x == lX) and (run < MAX_STAYS or x == lX):
            opts.append((abs(x - y - 1 - target[x + y + 1]), 1 + rng.random(), "Y"))
        step = min(opts, key=lambda o: (o[0] if o[1] >= 0 else -1, o[1]))[2]
        run = run + 1 if step == "Y" and last == "Y" else (1 if step == "Y" else 0)
        last = step
        if last == "M":
            ev_kmer.append(x)
            x += 1
            y += 1
        elif last == "X":
            x += 1
        else:
            ev_kmer.append(x - 1)
            y += 1
        cells.append((x, y))
    return np.array(ev_kmer, np.int64), np.array(cells, np.int64)


def emit(rng, match, kidx, ev_kmer):
    """events of a path, as make_read emits them (per-read affine rescaling of the pore model)"""
    lY = len(ev_kmer)
    scale, shift = rng.uniform(0.95, 1.05), rng.uniform(-5.0, 5.0)
    var, scale_sd, var_sd = rng.uniform(0.9, 1.1), rng.uniform(0.9, 1.2), rng.uniform(0.9, 1.2)
    scaled = synth.scale_model(match, scale, shift, var, scale_sd, var_sd)
    t = scaled[1:].reshape(synth.NUM_KMERS, 5)[kidx[ev_kmer]]
    events = np.zeros((lY, 3))
    events[:, 0] = rng.normal(t[:, 0], t[:, 1])
    events[:, 1] = np.maximum(np.abs(rng.normal(t[:, 2], t[:, 3])), 1e-3)
    events[:, 2] = rng.exponential(0.01, lY)
    return events, scaled, (scale, shift, var, scale_sd, var_sd)


def plan(rng, lX, lY, every, width, skip=None, e=None):
    """(anchors, expansion, nominal counts) of a read whose widest band is exactly `width` k-mers (the expansion is even: widths step
    by two with it, so a nominal path of the wrong parity is drawn again); with e given, a read whose widest band at
    that expansion is at most `width`"""
    for k in range(64):
        sk = None if skip is None else (skip[0], skip[1], skip[2] + k % 4)  # (the dwell sets the parity)
        counts = nominal_counts(rng, lX, lY, sk)
        an = anchors_of(counts, every, sk)
        if e is not None:
            if widest(an, lX, lY, e) <= width:
                return an, e, counts
            continue
        e0 = 2 * max(1, (width - 2 * every) // 2)
        ew = e0 + width - widest(an, lX, lY, e0)
        if ew >= 0 and ew % 2 == 0 and widest(an, lX, lY, ew) == width:
            return an, ew, counts
    raise ValueError("no nominal path gives a band %d k-mers wide" % width)


def emit_hdp(rng, seq_bytes, ev_kmer, hdp):
    """events of a path for the HDP machine, as harness.hdp_batch draws them: around the mode of each k-mer's HDP
    density.  hdp = (the nhdp dict of pyoracle.load_nhdp, the oracle's HdpModel)"""
    nhdp, model = hdp
    x = seq_bytes.decode()
    mode = {}
    events = np.zeros((len(ev_kmer), 3))
    for j, k in enumerate(ev_kmer):
        if k not in mode:
            row = nhdp["kmer_row"][model.kmer_id(x[k:k + 6])]
            mode[k] = nhdp["grid"][int(np.argmax(nhdp["y"][row]))]
        events[j] = (mode[k] + rng.normal(0, HDP_SD), abs(rng.normal(1.0, 0.2)) + 1e-3, 0.01)
    return events


def edge_read(rng, match, lX, lY, e, place, offset=0, every=4, width=None, cross=None, skip=None, centred=False,
              hdp=None):
    """One strand whose path runs `offset` cells inside the `place` edge of its band ('lower', 'upper', or 'cross'
    with cross = (d0, d1) as fractions of the diagonals).  With width set and e None, the expansion is chosen to make
    the widest band exactly that many k-mers; with both set, the widest band at expansion e is at most `width`.
    centred: the same sequence and anchors (so the same band), the events emitted from the nominal path the anchors
    sit on instead: the mass down the middle of the band.  hdp: events for the HDP machine (emit_hdp).
    Returns make_read's dict plus the expansion and the band."""
    seq = rng.integers(0, 4, lX + 5).astype(np.uint8)
    seq_bytes = bytes(np.frombuffer(b"ACGT", np.uint8)[seq])
    kidx = synth.kmer_indices(seq_bytes)
    if width is not None:
        anchors, e, counts = plan(rng, lX, lY, every, width, skip, e)
    else:
        counts = nominal_counts(rng, lX, lY, skip)
        anchors = anchors_of(counts, every, skip)
    L, R = o.band(anchors, lX, lY, e)
    if cross is not None:
        cross = (int(cross[0] * (lX + lY)), int(cross[1] * (lX + lY)))
    target = np.concatenate([target_of(L, R, place, offset, cross), [0, 0]])
    ev_kmer, cells = walk(rng, lX, lY, target)
    if centred:
        ev_kmer, cells = np.repeat(np.arange(lX), counts), None
    if hdp is not None:
        return dict(seq=seq_bytes, events=emit_hdp(rng, seq_bytes, ev_kmer, hdp), anchors=anchors, ev_kmer=ev_kmer,
                    cells=cells, e=e, L=L, R=R)
    events, scaled, params = emit(rng, match, kidx, ev_kmer)
    return dict(seq=seq_bytes, events=events, anchors=anchors, scaled_match=scaled, scale_params=params,
                ev_kmer=ev_kmer, cells=cells, e=e, L=L, R=R)


def edge_batch(seed, n, lX, lY, place, offset=0, every=4, e=40, width=None, cross=None, skip=None,
               model_seed=synth.SEED0, centred=False, hdp=None):
    """make_batch's layout (one scaled model per read) for n edge reads; every read gets the same expansion (the
    first read's when width is set: its band is then exactly `width` wide, the others' at most that).  centred: the
    same band, the mass in its middle (edge_read).  hdp: reads for the HDP machine, one model (id 0) shared, the
    sequences as text (harness.hdp_batch's layout)"""
    match, gap_x, gap_y = synth.synthetic_pore_model(model_seed)
    xs, evs, ans, items, models = [], [], [], [], []
    xo = yo = ao = 0
    for r in range(n):
        rng = np.random.default_rng(synth.SEED0 + seed * 1000 + r)
        rd = edge_read(rng, match, lX, lY, None if width is not None and r == 0 else e, place, offset, every, width,
                       cross, skip, centred, hdp)
        if r == 0:
            e = rd["e"]
        xs.append(rd["seq"])
        evs.append(rd["events"])
        ans.append(rd["anchors"])
        if hdp is None:
            models.append((rd["scaled_match"], gap_x, gap_y))
        items.append(dict(x_offset=xo, lX=lX, y_offset=yo, lY=lY, anchor_offset=ao, n_anchors=len(rd["anchors"]),
                          model=0 if hdp is not None else r))
        xo += lX + 5
        yo += lY
        ao += len(rd["anchors"])
    if hdp is not None:
        return dict(x_chars=b"".join(xs).decode(), events=np.concatenate(evs), anchors=np.concatenate(ans),
                    items=items, e=e)
    return dict(x_chars=b"".join(xs), events=np.concatenate(evs), anchors=np.concatenate(ans), items=items,
                models=models, base_model=(match, gap_x, gap_y), e=e)


def edge_mass(batch, i, bp, ragged=(0, 0), transitions=None):
    """the oracle's cell dump of item i of a batch as per-diagonal arrays, a dict: dump (the oracle's), match[d] the
    match posterior exp(F + B - total) of diagonal d's cells from xmin up (total: the window's, as the reference
    refreshes it every ten decoded diagonals), gapx[d] the same of gap X, cell[d] the cells' posterior summed over the
    states, xmin[d] the diagonal's least x, seg[d] the diagonal at which the total that covers d was refreshed"""
    from harness import run_oracle_item
    return _state_mass(run_oracle_item(batch, i, bp, ragged, transitions=transitions, dump=True))


def vanilla_edge_mass(batch, i, model, bp, ragged=(0, 0)):
    """edge_mass of item i under the vanilla machine: the oracle's cell dump with `model` (an o.VanillaModel, whose
    states are match, gap X, gap Y as the strawMan machine's)"""
    from harness import orc_params
    it = batch["items"][i]
    x = batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5]
    ev = batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]]
    an = batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]]
    return _state_mass(o.banded_dump(model, x, it["lX"], ev, an, orc_params(bp, split=1 << 60), ragged[0], ragged[1]))


def _state_mass(dump):
    txay = np.asarray(dump["totals_xay"])
    tval = np.asarray(dump["totals"])
    order = np.argsort(txay)
    txay, tval = txay[order], tval[order]
    F, B, L, R, off = dump["F"], dump["B"], dump["L"], dump["R"], dump["offsets"]
    nd = len(L)
    seg = np.searchsorted(txay, np.arange(nd))  # the refresh (of the total) that covers each diagonal
    match, gapx, cell, xmin = [], [], [], []
    for d in range(nd):
        tot = tval[min(seg[d], len(tval) - 1)]
        c = slice(off[d], off[d + 1])
        p = np.exp(F[c] + B[c] - tot)
        match.append(p[:, 0])
        gapx.append(p[:, 1])
        cell.append(p.sum(axis=1))
        xmin.append((d + int(L[d])) // 2)
    return dict(dump=dump, match=match, gapx=gapx, cell=cell, xmin=np.array(xmin),
                seg=txay[np.minimum(seg, len(txay) - 1)])


def edge_fraction(m, place, thr, reach=1, skip_ends=0, kind="match"):
    """fraction of the diagonals d > 0 (less `skip_ends` at either end) whose cell on the `place` edge ('lower':
    xmin, 'upper': xmax), or one within `reach` cells of it, has posterior >= thr: of the match state (kind 'match')
    or of the cell, all states together ('cell')"""
    nd = len(m[kind])
    hit = n = 0
    for d in range(1 + skip_ends, nd - skip_ends):
        p = m[kind][d]
        cells = p[:reach + 1] if place == "lower" else p[-(reach + 1):]
        n += 1
        hit += bool(cells.max() >= thr)
    return hit / max(n, 1)


SLOT_PERIODS = (128, 192, 256, 384, 512)  # WV_P of the two wave builds, SY_P of the three workgroup builds


def slot_period(build):
    """the slot period of a build, given as the wave family's cells per lane (2, 3: 64 slots each) or as the period
    itself (one of SLOT_PERIODS)"""
    P = 64 * build if build < 64 else build
    assert P in SLOT_PERIODS, build
    return P


def column_skip_bin(seq, match, x):
    """the skip bin of column x (the cells that have consumed x k-mers) on a read's scaled match table, as skip_bin in
    oracle/cpecan_oracle.c takes it through get_symbols: min(29, int(|level(k) - level(k_prev)| / 0.5)) of the k-mers
    at max(x - 2, 0) and one past it"""
    kidx = synth.kmer_indices(seq)
    p = max(x - 2, 0)
    level = np.asarray(match)[1:].reshape(synth.NUM_KMERS, 5)[:, 0]
    return min(29, int(abs(level[kidx[p + 1]] - level[kidx[p]]) / 0.5))


def a_record_slots(m, cells_per_lane, floor=1e-3):
    """the fused E-step's A-record condition on an oracle dump (edge_mass): refresh segments (the decoded diagonals
    that share one total) in which one slot of the kernel (column x mod P, P = slot_period(cells_per_lane): the wave
    builds' WV_P, or given directly the workgroup builds' SY_P -- there a slot holds the forward cell of column
    x mod SY_P and points at column x + 1 (SY_SLOT, gCol), and two columns P apart share a slot under any such fixed
    shift) holds two columns of the band, the higher one (the sweep back meets it first, and moves the slot on from
    it) with gap-X posterior >= floor summed over the segment.  The issue that asked for this condition wants gap-X mass on both columns; the
    kernel's store (cpecan_kernel_wave.hip, `x != cA[j]`) fires whenever the slot moves on from a column whose sum is
    non-zero, whatever the new column holds, and a lost A record loses the higher column's sum only, so the lower
    column has only to be in the band here.  Returns a list of (segment's top diagonal, slot, higher column, its gap-X
    mass, lower column)."""
    P = slot_period(cells_per_lane)
    segs = {}
    for d in range(1, len(m["gapx"])):
        g = m["gapx"][d]
        seg = segs.setdefault(int(m["seg"][d]), {})
        for x, v in zip(m["xmin"][d] + np.arange(len(g)), g):
            col = seg.setdefault(int(x) % P, {})
            col[int(x)] = col.get(int(x), 0.0) + float(v)
    out = []
    for top, seg in sorted(segs.items()):
        for slot, cols in seg.items():
            if len(cols) > 1 and cols[max(cols)] >= floor:
                out.append((top, slot, max(cols), cols[max(cols)], min(cols)))
    return out


# ---------------------------------------------- the case families ----------------------------------------------
# name -> edge_batch arguments and what the coverage test asserts on the oracle (tests/test_band_edges_cpu.py):
# `frac` of the decoded diagonals have posterior >= 0.01 (the cell's, all states) on the `place` edge or one cell
# inside it; `width` the widest band; `arec` the cells per lane of the wave build whose A-record condition must occur
FAMILY = dict(lX=200, lY=300, every=1, e=40, md=100, tb=40, ragged=(0, 0), offset=0, frac=0.25, width=None,
              cross=None, skip=None, arec=None, seed=1)


def _f(**kw):
    return dict(FAMILY, **kw)


FAMILIES = {
    "lower": _f(place="lower", ragged=(1, 1), frac=0.25),
    "lower1": _f(place="lower", offset=1, frac=0.25),
    "upper": _f(place="upper", frac=0.5),
    "upper1": _f(place="upper", offset=1, ragged=(1, 1), frac=0.5),
    "lower-out": _f(place="lower", offset=-2, ragged=(1, 0), frac=0.02),
    "upper-out": _f(place="upper", offset=-2, ragged=(0, 1), frac=0.05),
    "cross": _f(place="cross", cross=(0.45, 0.5), md=60, tb=30, ragged=(1, 1), frac=0.05),
}
for _w in (56, 57, 120, 121, 158, 159, 184, 185, 248, 249):  # each build's widest band and one k-mer past it
    FAMILIES["w%d" % _w] = _f(place="upper", lX=300, lY=450, width=_w, md=150, tb=40, ragged=(_w % 2, 1))
FAMILIES["arec120"] = _f(place="upper", lX=300, lY=500, width=120, skip=(150, 30, 1), md=150, tb=40, ragged=(1, 1),
                         arec=2)
FAMILIES["arec184"] = _f(place="upper", lX=300, lY=500, width=184, skip=(150, 30, 1), md=150, tb=40, ragged=(1, 1),
                         arec=3, seed=2)


def family_batch(name, n=2, seed=None, centred=False, hdp=None):
    f = FAMILIES[name]
    return edge_batch(f["seed"] if seed is None else seed, n, f["lX"], f["lY"], f["place"], f["offset"],
                      every=f["every"], e=f["e"], width=f["width"], cross=f["cross"], skip=f["skip"], centred=centred,
                      hdp=hdp)


# ------------------------------------------------ DNA (5-state) ------------------------------------------------
# The same path-first construction for the 5-state symbol machine (DNA against DNA): x is lX bases (no pad), y the
# bases the path emits.  A match step copies x's base into y (a substitution with probability DNA_SUB), a gap-Y step
# inserts a random base, a gap-X step deletes x's base.  Bands are in cells of the (lX + 1) x (lY + 1) matrix.
DNA_SUB = 0.02
# the widest band of each 5-state build (cells): the wave5 kernels at one, two, three cells per lane; the general
# kernel keeps its diagonals in LDS up to DNA_LDS, in HBM past it; its workgroup has 256 threads
DNA_WAVE_L1, DNA_WAVE_L2, DNA_WAVE_L3, DNA_LDS, GENERAL_THREADS = 64, 128, 192, 248, 256


def dna_y(rng, xb, cells):
    """the bases a path (walk's cells, (0, 0) first) emits against x (0..3 codes)"""
    y = []
    for (x0, y0), (x1, y1) in zip(cells[:-1], cells[1:]):
        if y1 == y0:
            continue  # gap X: x's base deleted
        if x1 == x0:
            y.append(int(rng.integers(0, 4)))  # gap Y: an inserted base
        elif rng.random() < DNA_SUB:
            y.append(int((xb[x0] + rng.integers(1, 4)) % 4))
        else:
            y.append(int(xb[x0]))
    return np.array(y, np.int64)


def nominal_cells(counts):
    """the nominal path of `counts` (nominal_counts) as cells: base x is matched to the first of its counts[x] y's and
    the others inserted after it; counts[x] = 0 deletes it"""
    x = y = 0
    cells = [(0, 0)]
    for c in counts:
        if c == 0:
            x += 1
        else:
            x, y = x + 1, y + 1
        cells.append((x, y))
        for _ in range(int(c) - 1):
            y += 1
            cells.append((x, y))
    return np.array(cells, np.int64)


def dna_read(rng, lX, lY, e, place, offset=0, every=4, width=None, cross=None, centred=False):
    """one DNA pair (x, y) whose path runs as edge_read's does; centred: the same x and anchors (so the same band), y
    emitted from the nominal path the anchors sit on.  Returns a dict: x, y (strings), anchors, cells (the path), e,
    L, R"""
    xb = rng.integers(0, 4, lX)
    if width is not None:
        anchors, e, counts = plan(rng, lX, lY, every, width, None, e)
    else:
        counts = nominal_counts(rng, lX, lY)
        anchors = anchors_of(counts, every)
    L, R = o.band(anchors, lX, lY, e)
    if cross is not None:
        cross = (int(cross[0] * (lX + lY)), int(cross[1] * (lX + lY)))
    target = np.concatenate([target_of(L, R, place, offset, cross), [0, 0]])
    _, cells = walk(rng, lX, lY, target)
    if centred:
        cells = nominal_cells(counts)
    yb = dna_y(rng, xb, cells)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    return dict(x=bytes(acgt[xb]).decode(), y=bytes(acgt[yb]).decode(), anchors=anchors, cells=cells, e=e, L=L, R=R)


DNA_FAMILY = dict(lX=300, lY=300, every=1, e=40, md=100, tb=40, ragged=(0, 0), offset=0, frac=0.25, width=None,
                  cross=None, seed=1)


def _d(**kw):
    return dict(DNA_FAMILY, **kw)


# name -> dna_batch arguments and what test_band_edges_cpu.py asserts on the oracle's dump (as FAMILIES)
DNA_FAMILIES = {
    "lower": _d(place="lower", ragged=(1, 1), frac=0.5),
    "lower1": _d(place="lower", offset=1, frac=0.5),
    "upper": _d(place="upper", frac=0.5),
    "upper1": _d(place="upper", offset=1, ragged=(1, 1), frac=0.5),
    "lower-out": _d(place="lower", offset=-2, ragged=(1, 0), frac=0.15),
    "upper-out": _d(place="upper", offset=-2, ragged=(0, 1), frac=0.15),
    "cross": _d(place="cross", cross=(0.45, 0.5), md=60, tb=30, ragged=(1, 1), frac=0.05),
}
for _w in (64, 65, 128, 129, 192, 193, 248, 249, 256, 257):  # each 5-state build's widest band and one cell past it
    DNA_FAMILIES["w%d" % _w] = _d(place="upper", lX=380, lY=380, width=_w, md=150, tb=40, ragged=(_w % 2, 1),
                                  frac=0.5)


def dna_batch(name, n=2, seed=None, centred=False):
    """n reads of DNA family `name` (every read at the first one's expansion) as test_dna5_gpu.run_case takes them:
    dict(seqs=[(x, y, anchors)], e, reads)"""
    f = DNA_FAMILIES[name]
    seed = f["seed"] if seed is None else seed
    e, seqs, reads = f["e"], [], []
    for r in range(n):
        rng = np.random.default_rng(synth.SEED0 + 500000 + seed * 1000 + r)
        rd = dna_read(rng, f["lX"], f["lY"], None if f["width"] is not None and r == 0 else e, f["place"],
                      f["offset"], f["every"], f["width"], f["cross"], centred)
        e = rd["e"]
        seqs.append((rd["x"], rd["y"], rd["anchors"]))
        reads.append(rd)
    return dict(seqs=seqs, e=e, reads=reads)


def dna_edge_mass(x, y, anchors, bp, ragged=(0, 0)):
    """edge_mass's per-diagonal cell posteriors (all five states) of one DNA pair on the oracle's dump"""
    from harness import orc_params
    dump = o.banded_dump(o.Sm5Model(), x, len(x), y, anchors, orc_params(bp, split=1 << 60), ragged[0], ragged[1])
    return _cell_mass(dump)


def _cell_mass(dump):
    txay = np.asarray(dump["totals_xay"])
    order = np.argsort(txay)
    txay, tval = txay[order], np.asarray(dump["totals"])[order]
    F, B, off = dump["F"], dump["B"], dump["offsets"]
    seg = np.searchsorted(txay, np.arange(len(dump["L"])))
    cell = [np.exp(F[off[d]:off[d + 1]] + B[off[d]:off[d + 1]] - tval[min(seg[d], len(tval) - 1)]).sum(axis=1)
            for d in range(len(dump["L"]))]
    return dict(dump=dump, cell=cell)


# ------------------------------------ signal families for the other machines ------------------------------------
# the general kernels' 256-thread chunking (cpecan_general.h) and their 64-lane waves: a band of exactly 256 (64)
# k-mers and one past it, for the 4-state and echelon machines (make_batch's layout, as FAMILIES; kept apart so that the strawMan tests do not run them)
WIDE_FAMILIES = {"w%d" % _w: _f(place="upper", lX=300, lY=450, width=_w, md=150, tb=40, ragged=(_w % 2, 1))
                 for _w in (64, 65, 256, 257)}


# the vanilla machine's workgroup builds (SY_P = 256, 384, 512 slots for bands of up to 248, 376, 504 k-mers), kept
# apart as WIDE_FAMILIES is.  varec...: the A-record condition at the build's slot period (`arec`): a band within a few
# k-mers of the period that crosses 30 skipped k-mers in the middle of the read, 700 k-mers long so that the band has
# that many columns to cross.  vlower...: the path on the band's lower edge at the build's widest band
# (test_vanilla_workgroup_gpu.exact_width_batch is the same read on the upper edge).
VANILLA_FAMILIES = {}
for _w in (248, 376, 504):
    VANILLA_FAMILIES["varec%d" % _w] = _f(place="upper", lX=700, lY=1050, width=_w, skip=(350, 30, 1), md=150, tb=40,
                                          ragged=(1, 1), arec=_w + 8)
    VANILLA_FAMILIES["vlower%d" % _w] = _f(place="lower", lX=700, lY=1050, width=_w, md=150, tb=40,
                                           ragged=(_w % 2, 1))


def signal_family(name):
    for families in (FAMILIES, WIDE_FAMILIES, VANILLA_FAMILIES):
        if name in families:
            return families[name]
    raise KeyError(name)


def signal_batch(name, n=2, seed=None, centred=False):
    """family_batch for a family of FAMILIES or WIDE_FAMILIES"""
    f = signal_family(name)
    return edge_batch(f["seed"] if seed is None else seed, n, f["lX"], f["lY"], f["place"], f["offset"],
                      every=f["every"], e=f["e"], width=f["width"], cross=f["cross"], skip=f["skip"], centred=centred)


def echelon_reads(batch, seed):
    """a thin adapter for the echelon machine: a signal batch (signal_batch) as test_echelon_gpu.reads' reads, each
    with its own machine (its scaled pore model, skip bins of its own) and event durations drawn as that test draws
    them (the batch itself is left as it is).  The echelon machine does not follow the batch's path (its match
    emission carries almost nothing of the event's level), so these reads give its kernel the batch's band widths, not
    mass on the band's edge.  Returns [dict(seq, events, anchors, machine)]"""
    import echelon_dp
    _, _, gap_y = batch["base_model"]
    out = []
    for r, it in enumerate(batch["items"]):
        rng = np.random.default_rng(synth.SEED0 + 700000 + seed * 1000 + r)
        ev = batch["events"][it["y_offset"]: it["y_offset"] + it["lY"]].copy()
        ev[:, 2] = rng.uniform(0.0008, 0.012, it["lY"])
        skip = np.sort(rng.uniform(0.05, 0.4, 30))[::-1]
        out.append(dict(seq=batch["x_chars"][it["x_offset"]: it["x_offset"] + it["lX"] + 5], events=ev,
                        anchors=batch["anchors"][it["anchor_offset"]: it["anchor_offset"] + it["n_anchors"]],
                        machine=echelon_dp.Machine(batch["models"][it["model"]][0], np.concatenate([skip, skip]),
                                                   gap_y)))
    return out

