"""A layout across many calls.  Since round 3 a layout carries state from one call to the next: arrival cells that the
last party of a scan leaves at zero, expanded scan groups and the narrow-group list (rebuilt when the descriptors
change, re-cut when scan_tiles_per_wg changes), tile records (rebuilt when dirty), the width hint that picks the encode
form of 4-byte columns, the single-pass encode's look-back words and the selection scan's shared-word records.  Bugs in
that state show only on the NEXT call of the same layout, so these tests keep layouts alive through re-encodes,
descriptor reloads, relocations, knob flips and rejected calls, and check every read path after every step.  Expected
results come from numpy and the C oracle only, never from an earlier GPU read."""
import numpy as np
import pytest

from test_gpu_parity import ALL_DTYPES, U64, check_placement, make_values, oracle_encode, wide_sum
from test_gpu_select import bit_pattern, pack_mask

pytestmark = pytest.mark.gpu

POISON = 0xDEADBEEFDEADBEEF
DEFAULT_KNOBS = {"scan_tiles_per_wg": 0, "scan_cells": 1, "templated_scan": 1, "tile_records": 1,
                 "single_pass_encode": 1, "encode_placement": 0, "sel_debug": 0}
MAX_SHIFT = 4   # a relocated arena starts 16 * k words into its buffer, k <= MAX_SHIFT


def set_knobs(adac, knobs):
    for k, v in knobs.items():
        adac.set_tuning(k, v)


def expected_decode(adac, orc, enc, n, dtype):
    """What a segment decodes to: the oracle's own packed words unpacked (NULL slots included)."""
    mn, mx, w, packed, words = enc
    smin = adac.stored_min(mn, mx, w) if packed else mn
    add = smin if (packed and smin != U64) else 0
    return orc.unpack_flat(words, 0, n, w, add, dtype)


def valid_mask(rng, span, counts, offs):
    """Random validity over the element index space; every segment with rows keeps one valid row (an all-NULL segment
    is covered by test_gpu_parity.test_nulls_validity_mask)."""
    valid = rng.random(span) > rng.random() * 0.7
    for c, o in zip(counts, offs):
        if c:
            valid[o + int(rng.integers(0, c))] = True
    return valid


class Col:
    """One layout, two word buffers (a relocation copies the arena into the other one) and the model every read of it
    is checked against."""

    def __init__(self, adac, ctx, dtype, counts, offs, dense):
        self.dtype = np.dtype(dtype)
        self.isz = self.dtype.itemsize
        self.counts = np.array(counts, dtype=np.uint32)
        self.offs = [int(o) for o in offs]
        self.offs_u64 = np.array(self.offs, dtype=np.uint64)
        self.lay = adac.Layout(ctx, self.dtype, self.counts, None if dense else self.offs_u64)
        self.span = int(self.lay.value_span)
        self.maw = int(self.lay.max_arena_words)
        self.nwords = self.maw + 16 * MAX_SHIFT + 16
        self.bufs = [ctx.alloc(self.nwords * 8), ctx.alloc(self.nwords * 8)]
        self.which, self.shift = 0, 0
        self.enc = self.dec = self.valid = None   # oracle encode, decoded model, validity of the last encode
        nseg = len(self.counts)
        self.nz = [s for s in range(nseg) if self.counts[s]]
        self.out_words = (max(self.span, 64) * self.isz + 64 + 7) // 8   # >= 64 point fetches
        self.d_out = ctx.alloc(self.out_words * 8)
        self.d_aux = ctx.alloc((max(self.span, 1) + 8) * 8)
        self.d_res = ctx.alloc(nseg * 8 + 8)
        self.d_bm = ctx.alloc(((self.span + 63) // 64 + 1) * 8)

    @property
    def d_words(self):
        return self.bufs[self.which]

    def poison_words(self):
        self.d_words.upload(np.full(self.nwords, POISON, dtype=np.uint64))


def make_shape(rng, adac, dtype):
    dtype = np.dtype(dtype)
    tile = adac.tile_values(dtype)
    if rng.random() < 0.15:   # hundreds of tiny segments: many groups share one bitmap word
        counts = [int(x) for x in rng.integers(0, 40, size=int(rng.integers(200, 401)))]
        counts[int(rng.integers(0, len(counts)))] = 33
    else:
        pool = [0, 1, 31, 32, 33, 63, 64, 65, tile - 1, tile, tile + 1]
        counts = []
        for _ in range(int(rng.integers(1, 9))):
            r = rng.random()
            counts.append(int(rng.choice(pool)) if r < 0.6 else int(rng.integers(2, 3 * tile)) if r < 0.85
                          else int(rng.integers(3 * tile, 20 * tile)))
    if not any(counts):
        counts[0] = 65
    dense = bool(rng.random() < 0.5)
    offs, run = [], 0
    for c in counts:
        if not dense:
            run += int(rng.integers(0, 40))
        offs.append(run)
        run += c
    return counts, offs, dense


def seg_widths(rng, tb, n):
    ws = sorted({1, 2, 3, 4, 7, 8, 13, 17, 18, 24, 31, 32, 33, 48, tb - 1, tb} & set(range(1, tb + 1)))
    return [int(rng.choice(ws)) for _ in range(n)]


def check_encoded(adac, col, first_come, with_minmax=True):
    """Descriptors, min/max and the words at every descriptor's own word_off against the oracle's encode."""
    descs = col.lay.get_descs()
    mm = col.lay.get_minmax()
    words_all = col.d_words.download(np.uint64, col.nwords)
    woff = 0
    for s, (mn, mx, w, packed, ew) in enumerate(col.enc):
        d = descs[s]
        n = int(col.counts[s])
        assert int(d["count"]) == n and int(d["val_off"]) == col.offs[s], s
        assert int(d["width"]) == w, "width of segment %d" % s
        assert bool(d["flags"] & adac.SEG_PACKED) == packed, "flags of segment %d" % s
        if packed:
            assert int(d["min"]) == adac.stored_min(mn, mx, w), "min of segment %d" % s
        if with_minmax and n:
            assert (int(mm[s, 0]), int(mm[s, 1])) == (mn, mx), "min/max of segment %d" % s
        if not first_come:
            assert int(d["word_off"]) == woff, "ordered offset of segment %d" % s
        woff += adac.arena_words(n, w)
        a = int(d["word_off"])
        assert np.array_equal(words_all[a:a + len(ew)], ew), "packed words of segment %d (w=%d)" % (s, w)
    check_placement(adac, descs, col.maw)
    return descs


def check_reads(adac, ctx, col, rng, tag):
    """Every read path of the layout against the model, every output poisoned before its call."""
    dt, isz, span, lay, d_words = col.dtype, col.isz, col.span, col.lay, col.d_words
    nseg = len(col.counts)
    udt = np.dtype("u%d" % isz)
    dec, offs = col.dec, col.offs
    poison_vals = np.full(col.out_words, POISON, dtype=np.uint64)
    n_out = col.out_words * 8 // isz
    # full decode
    col.d_out.upload(poison_vals)
    lay.unpack(d_words, col.d_out)
    out = col.d_out.download(dt, n_out)
    for s in col.nz:
        assert np.array_equal(out[offs[s]:offs[s] + len(dec[s])], dec[s]), (tag, "unpack", s)
    assert np.all(out[span:].view(udt) == poison_vals.view(udt)[span:n_out]), (tag, "unpack wrote past the span")
    # one range, at an output offset
    s = col.nz[int(rng.integers(0, len(col.nz)))]
    c = int(col.counts[s])
    start = int(rng.integers(0, c))
    cnt = int(rng.integers(1, c - start + 1))
    shift = int(rng.integers(0, 3)) * (16 // isz)
    col.d_out.upload(poison_vals)
    lay.unpack_range(d_words, s, start, cnt, col.d_out, shift)
    got = col.d_out.download(dt, shift + cnt + 1)
    assert np.array_equal(got[shift:shift + cnt], dec[s][start:start + cnt]), (tag, "unpack_range", s, start, cnt)
    assert np.all(got.view(udt)[:shift] == poison_vals.view(udt)[:shift]), (tag, "unpack_range before its offset")
    assert got.view(udt)[shift + cnt] == poison_vals.view(udt)[shift + cnt], (tag, "unpack_range past its count")
    # point fetch
    k = 64
    fs = np.array([col.nz[int(i)] for i in rng.integers(0, len(col.nz), size=k)], dtype=np.uint32)
    fr = np.array([int(rng.integers(0, col.counts[int(x)])) for x in fs], dtype=np.uint32)
    col.d_out.upload(poison_vals)
    lay.fetch_rows(d_words, ctx.upload(fs), ctx.upload(fr), k, col.d_out)
    exp = np.array([dec[int(a)][int(b)] for a, b in zip(fs, fr)], dtype=dt)
    assert np.array_equal(col.d_out.download(dt, k), exp), (tag, "fetch_rows")
    # layout-free jobs from the downloaded descriptors: a random range of every segment, at its own element offset
    descs = lay.get_descs()
    ranges, outs = [], []
    for s in col.nz:
        c = int(col.counts[s])
        st = int(rng.integers(0, c))
        ranges.append((st, int(rng.integers(0, c - st + 1))))
        outs.append(offs[s] + st)
    jobs = adac.jobs_from_descs([descs[s] for s in col.nz], ranges, outs)
    col.d_out.upload(poison_vals)
    adac.unpack_jobs(ctx, dt, jobs, d_words, col.d_out)
    out = col.d_out.download(dt, max(span, 1))
    for s, (st, c) in zip(col.nz, ranges):
        assert np.array_equal(out[offs[s] + st:offs[s] + st + c], dec[s][st:st + c]), (tag, "unpack_jobs", s, st, c)
    # fused scans, with and without validity (the encode's own mask when it had one)
    pool = np.concatenate([dec[s] for s in col.nz])
    a, b = sorted((pool[int(rng.integers(0, len(pool)))], pool[int(rng.integers(0, len(pool)))]))
    info = np.iinfo(dt)
    lo, hi = [(int(a), int(b)), (int(info.min), int(b)), (int(a), int(info.max))][int(rng.integers(0, 3))]
    nw = (span + 63) // 64
    res_poison = np.full(nseg + 1, POISON, dtype=np.uint64)
    vmask = col.valid if col.valid is not None else valid_mask(rng, span, col.counts, offs)
    for valid in (None, vmask):
        d_valid = None if valid is None else ctx.upload(pack_mask(valid, span))
        ok = [np.ones(len(dec[s]), bool) if valid is None else valid[offs[s]:offs[s] + len(dec[s])] for s in range(nseg)]
        vt = (tag, "valid" if valid is not None else "all")
        col.d_res.upload(res_poison)
        lay.scan_sum(d_words, col.d_res, d_valid)
        got = col.d_res.download(np.uint64, nseg + 1)
        assert got[:nseg].tolist() == [wide_sum(dec[s][ok[s]]) for s in range(nseg)], vt + ("sum",)
        assert int(got[nseg]) == POISON, vt + ("sum wrote past nseg",)
        sel = np.zeros(span, dtype=bool)
        for s in range(nseg):
            sel[offs[s]:offs[s] + len(dec[s])] = (dec[s] >= lo) & (dec[s] <= hi) & ok[s]
        want = [int(sel[offs[s]:offs[s] + len(dec[s])].sum()) for s in range(nseg)]
        col.d_res.upload(res_poison)
        lay.scan_count_between(d_words, bit_pattern(lo, dt), bit_pattern(hi, dt), col.d_res, d_valid)
        assert col.d_res.download(np.uint64, nseg).tolist() == want, vt + ("count_between", lo, hi)
        col.d_res.upload(res_poison)
        col.d_bm.upload(np.full(nw + 1, POISON, dtype=np.uint64))
        lay.scan_select_between(d_words, bit_pattern(lo, dt), bit_pattern(hi, dt), col.d_bm, col.d_res, d_valid)
        assert col.d_res.download(np.uint64, nseg).tolist() == want, vt + ("select counts", lo, hi)
        bm = col.d_bm.download(np.uint64, nw + 1)
        assert int(bm[nw]) == POISON, vt + ("bitmap sentinel",)
        exp_bm = pack_mask(sel, span)[:nw]   # tail bits past the span are zero in it
        bad = np.flatnonzero(bm[:nw] != exp_bm)
        assert bad.size == 0, vt + ("bitmap words", lo, hi, bad[:8].tolist())
    # COUNT(v = key)
    kv = pool[int(rng.integers(0, len(pool)))]
    col.d_res.upload(res_poison)
    lay.scan_count_eq(d_words, bit_pattern(kv, dt), col.d_res)
    assert col.d_res.download(np.uint64, nseg).tolist() == [int((v == kv).sum()) for v in dec], (tag, "count_eq")
    # scan with selection: values and ids of the rows of the last bitmap (the expected one, built here)
    ids = np.flatnonzero(sel)
    col.d_bm.upload(pack_mask(sel, span)[:max(nw, 1)])
    col.d_out.upload(poison_vals)
    col.d_aux.upload(np.full((max(span, 1) * 8 + 64) // 8, POISON, dtype=np.uint64))
    n = lay.unpack_selected(d_words, col.d_bm, col.d_out, col.d_aux)
    assert n == len(ids), (tag, "unpack_selected total")
    model = np.zeros(max(span, 1), dtype=dt)
    for s in col.nz:
        model[offs[s]:offs[s] + len(dec[s])] = dec[s]
    got_v = col.d_out.download(dt, len(ids) + 1)
    got_i = col.d_aux.download(np.uint64, len(ids) + 1)
    assert np.array_equal(got_v[:len(ids)], model[ids]), (tag, "unpack_selected values")
    assert np.array_equal(got_i[:len(ids)], ids.astype(np.uint64)), (tag, "unpack_selected ids")
    assert int(got_i[len(ids)]) == POISON, (tag, "unpack_selected wrote past its total")


def encode_step(adac, orc, ctx, col, rng, sp, placement, peek, with_valid):
    """adac_encode of new values; the model is the oracle's encode of them."""
    tb = 8 * col.isz
    nseg = len(col.counts)
    segs = [make_values(rng, col.dtype, int(c), w) for c, w in zip(col.counts, seg_widths(rng, tb, nseg))]
    rule = adac.RULE_APPEND if rng.random() < 0.6 else adac.RULE_RECOMPACT
    padded = bool(rng.random() < 0.3)
    valid = valid_mask(rng, col.span, col.counts, col.offs) if with_valid else None
    vm = None if valid is None else pack_mask(valid, col.span)
    host = np.zeros(max(col.span, 1), dtype=col.dtype)
    for v, o in zip(segs, col.offs):
        host[o:o + len(v)] = v
    d_vals = ctx.upload(host)
    d_valid = None if vm is None else ctx.upload(vm)
    adac.set_tuning("single_pass_encode", sp)
    adac.set_tuning("encode_placement", placement)
    if peek:   # the host reads the descriptors first: the width hint of 4-byte columns follows them
        col.lay.get_descs()
    col.which, col.shift = int(rng.integers(0, 2)), 0
    col.poison_words()
    col.lay.encode(d_vals, col.d_words, d_valid, rule, padded)
    col.enc = oracle_encode(orc, segs, rule, padded, vm, col.offs_u64)
    col.dec = [expected_decode(adac, orc, e, len(v), col.dtype) for e, v in zip(col.enc, segs)]
    col.valid = valid
    for s in col.nz:   # the oracle's own round trip on the valid rows
        ok = np.ones(len(segs[s]), bool) if valid is None else valid[col.offs[s]:col.offs[s] + len(segs[s])]
        assert np.array_equal(col.dec[s][ok], segs[s][ok]), s
    check_encoded(adac, col, first_come=placement == 1)
    return "encode sp=%d place=%d peek=%d valid=%d rule=%d pad=%d" % (sp, placement, peek, with_valid, rule, padded)


def reencode_step(adac, orc, src, dst, rng):
    """packed -> packed into the twin layout with the other padding or the other rule."""
    rule = adac.RULE_APPEND if rng.random() < 0.6 else adac.RULE_RECOMPACT
    padded = bool(rng.random() < 0.5)
    use_valid = src.valid is not None and rng.random() < 0.7
    vm = pack_mask(src.valid, src.span) if use_valid else None
    d_valid = None if vm is None else src.lay.ctx.upload(vm)
    dst.which, dst.shift = int(rng.integers(0, 2)), 0
    dst.poison_words()
    src.lay.reencode(src.d_words, dst.lay, dst.d_words, d_valid, rule, padded)
    dst.enc = oracle_encode(orc, src.dec, rule, padded, vm, dst.offs_u64)
    dst.dec = [expected_decode(adac, orc, e, len(v), dst.dtype) for e, v in zip(dst.enc, src.dec)]
    dst.valid = src.valid if use_valid else None
    check_encoded(adac, dst, first_come=False, with_minmax=False)
    return "reencode valid=%d rule=%d pad=%d" % (use_valid, rule, padded)


def relocate_step(adac, col, rng):
    """The arena copied into the other buffer 16 * k words further on; descriptors handed back shifted as much."""
    k = int(rng.integers(0, MAX_SHIFT + 1))
    while 16 * k == col.shift:
        k = int(rng.integers(0, MAX_SHIFT + 1))
    old = col.d_words.download(np.uint64, col.nwords)
    new = np.full(col.nwords, POISON, dtype=np.uint64)
    new[16 * k:16 * k + col.maw] = old[col.shift:col.shift + col.maw]
    descs = col.lay.get_descs()
    descs["word_off"] = descs["word_off"] - np.uint64(col.shift) + np.uint64(16 * k)
    col.which ^= 1
    col.d_words.upload(new)
    col.shift = 16 * k
    col.lay.set_descs(descs)
    assert col.lay.get_descs().tobytes() == descs.tobytes()
    return "relocate to +%d" % (16 * k)


def reject_step(adac, col, other, rng):
    """A call that must fail: status INVALID_ARGUMENT, descriptors unchanged."""
    before = col.lay.get_descs()
    before_other = other.lay.get_descs()
    kind = int(rng.integers(0, 4))
    bad = before.copy()
    s = int(rng.integers(0, len(bad)))
    if kind == 0:
        bad[s]["word_off"] += np.uint64(8)    # not a multiple of 16
    elif kind == 1:
        bad[s]["count"] += np.uint32(1)       # not the layout's count
    elif kind == 2:
        bad[s]["width"] = 0
    with pytest.raises(adac.AdacError) as e:
        if kind == 3:   # packed -> packed between layouts of different shape
            col.lay.reencode(col.d_words, other.lay, other.d_words, None, adac.RULE_APPEND, False)
        else:
            col.lay.set_descs(bad)
    assert e.value.status == 1, e.value
    assert col.lay.get_descs().tobytes() == before.tobytes()
    assert other.lay.get_descs().tobytes() == before_other.tobytes()
    return "rejected call %d" % kind


@pytest.mark.parametrize("seed", range(40))
def test_layout_survives_a_random_life(adac, oracle, gpu_ctx, seed):
    """Stateful differential fuzz: twin layouts A / B of one type and shape (re-encoded into each other) and a third
    layout C of another type, their calls interleaved over 10 - 14 random steps — encodes in every form and placement,
    packed -> packed re-encodes, descriptor reloads and relocations, knob flips and rejected calls — and every read
    path of the touched layout after every step."""
    rng = np.random.default_rng(70_000 + seed)
    dt_ab = np.dtype(ALL_DTYPES[int(rng.integers(0, len(ALL_DTYPES)))])
    dt_c = np.dtype(ALL_DTYPES[int(rng.integers(0, len(ALL_DTYPES)))])
    while dt_c == dt_ab:
        dt_c = np.dtype(ALL_DTYPES[int(rng.integers(0, len(ALL_DTYPES)))])
    counts, offs, dense = make_shape(rng, adac, dt_ab)
    cur = Col(adac, gpu_ctx, dt_ab, counts, offs, dense)
    twin = Col(adac, gpu_ctx, dt_ab, counts, offs, dense)
    c3 = Col(adac, gpu_ctx, dt_c, *make_shape(rng, adac, dt_c))
    log = []

    def encode(col):
        return encode_step(adac, oracle, gpu_ctx, col, rng, int(rng.integers(0, 3)), int(rng.integers(0, 2)),
                           bool(rng.random() < 0.5), bool(rng.random() < 0.35))

    try:
        set_knobs(adac, DEFAULT_KNOBS)
        log.append(("A", encode(cur)))
        check_reads(adac, gpu_ctx, cur, rng, log[-1])
        log.append(("C", encode(c3)))
        check_reads(adac, gpu_ctx, c3, rng, log[-1])
        for _ in range(int(rng.integers(10, 15))):
            live = [c for c in (cur, twin, c3) if c.enc is not None]
            op = rng.choice(["encode", "encode", "reencode", "reencode", "reload", "relocate", "knob", "knob", "reject"])
            col = live[int(rng.integers(0, len(live)))]
            if op == "encode":
                what = encode(col)
            elif op == "reencode":
                what = reencode_step(adac, oracle, cur, twin, rng)
                col = twin
                cur, twin = twin, cur
            elif op == "reload":
                col.lay.set_descs(col.lay.get_descs())
                what = "set_descs(get_descs())"
            elif op == "relocate":
                what = relocate_step(adac, col, rng)
            elif op == "knob":
                name = rng.choice(["scan_tiles_per_wg", "scan_cells", "templated_scan", "tile_records"])
                val = int(rng.choice([0, 1, 2, 3, 7, 16, 19] if name == "scan_tiles_per_wg" else
                                     [0, 1, 3] if name == "tile_records" else [0, 1]))
                adac.set_tuning(str(name), val)
                what = "%s=%d" % (name, val)
            else:
                other = c3 if col is not c3 else cur
                what = reject_step(adac, col, other, rng)
            log.append(("A" if col is cur else "B" if col is twin else "C", what))
            check_reads(adac, gpu_ctx, col, rng, (len(log), log[-1]))
    except AssertionError as e:
        raise AssertionError("step %d of %s: %s" % (len(log), log, e)) from e
    finally:
        set_knobs(adac, DEFAULT_KNOBS)


def scan_battery(adac, ctx, lay, d_words, dt, segs, offs, span, probes, valid, tag, reps=3):
    """SUM, COUNT and the selection scan (with and without validity) repeated on poisoned outputs."""
    nseg = len(segs)
    nw = (span + 63) // 64
    d_res = ctx.alloc(nseg * 8 + 8)
    d_bm = ctx.alloc((nw + 1) * 8)
    res_poison = np.full(nseg + 1, POISON, dtype=np.uint64)
    bm_poison = np.full(nw + 1, POISON, dtype=np.uint64)
    for vmask in (None, valid):
        d_valid = None if vmask is None else ctx.upload(pack_mask(vmask, span))
        ok = [np.ones(len(v), bool) if vmask is None else vmask[o:o + len(v)] for v, o in zip(segs, offs)]
        sums = [wide_sum(v[k]) for v, k in zip(segs, ok)]
        expect = []
        for lo, hi in probes:
            sel = np.zeros(span, dtype=bool)
            for v, o, k in zip(segs, offs, ok):
                sel[o:o + len(v)] = (v >= lo) & (v <= hi) & k
            expect.append((lo, hi, [int(sel[o:o + len(v)].sum()) for v, o in zip(segs, offs)], pack_mask(sel, span)[:nw]))
        t = tag + ("valid" if vmask is not None else "all",)
        for rep in range(reps):
            d_res.upload(res_poison)
            lay.scan_sum(d_words, d_res, d_valid)
            got = d_res.download(np.uint64, nseg + 1)
            assert got[:nseg].tolist() == sums and int(got[nseg]) == POISON, t + ("sum", rep)
            for lo, hi, cnt, bm in expect:
                d_res.upload(res_poison)
                lay.scan_count_between(d_words, bit_pattern(lo, dt), bit_pattern(hi, dt), d_res, d_valid)
                assert d_res.download(np.uint64, nseg).tolist() == cnt, t + ("count", lo, hi, rep)
                d_res.upload(res_poison)
                d_bm.upload(bm_poison)
                lay.scan_select_between(d_words, bit_pattern(lo, dt), bit_pattern(hi, dt), d_bm, d_res, d_valid)
                assert d_res.download(np.uint64, nseg).tolist() == cnt, t + ("select counts", lo, hi, rep)
                got = d_bm.download(np.uint64, nw + 1)
                assert int(got[nw]) == POISON, t + ("bitmap sentinel", rep)
                bad = np.flatnonzero(got[:nw] != bm)
                assert bad.size == 0, t + ("bitmap", lo, hi, rep, bad[:8].tolist())


@pytest.mark.parametrize("dtype", [np.uint64, np.int32, np.uint16, np.uint8])
def test_scan_arrivals_past_256_groups(adac, oracle, gpu_ctx, dtype):
    """Segments of exactly 255, 256, 257 and 300+ scan groups (scan_tiles_per_wg = 1: one group per tile) next to small
    ones: SUM's arrival switches to add-wait-count above 256 parties (arrive_sum), COUNT and the selection bitmap to
    their many-party forms.  Narrow (w 2, 3), common and unpacked widths; u64 values near 2^64 so that the halves carry
    and SUM wraps.  Every call repeated on poisoned outputs (the cells must be back at zero), the default grouping
    interleaved on the same layout (the same cells switch between the <= 256 and > 256 forms), both kernel forms, and
    the clearing-pass form (scan_cells = 0) as the cross-check."""
    dt = np.dtype(dtype)
    tb = 8 * dt.itemsize
    tile = adac.tile_values(dt)
    rng = np.random.default_rng(256 + tb + (dt.kind == "i"))
    common = {64: 37, 32: 13, 16: 7, 8: 5}[tb]
    big = [255 * tile, 256 * tile - 1, 256 * tile + 1, 300 * tile + 77]   # 255, 256, 257, 301 groups at one tile each
    for rot in range(2):
        widths = [2, 3, common, tb][rot:] + [2, 3, common, tb][:rot]
        counts, ws = [], []
        for c, w in zip(big, widths):
            counts += [c, int(rng.integers(1, 70))]
            ws += [w, int(rng.integers(1, tb + 1))]
        counts.insert(1, 0)
        ws.insert(1, 1)
        segs = []
        for c, w in zip(counts, ws):
            base = None
            if tb == 64 and w < 64:
                base = 2 ** 64 - 2 ** (w + 1)   # near the top: sums of the halves carry, SUM wraps
            segs.append(make_values(rng, dt, c, w, base))
        counts = np.array(counts, dtype=np.uint32)
        lay = adac.Layout(gpu_ctx, dt, counts)
        offs = np.concatenate([[0], np.cumsum(counts[:-1])]).astype(np.int64).tolist()
        span = int(counts.sum())
        d_vals = gpu_ctx.upload(np.concatenate(segs))
        d_words = gpu_ctx.alloc(lay.max_arena_words * 8 + 64).zero()
        lay.encode(d_vals, d_words, None, adac.RULE_APPEND, False)
        enc = oracle_encode(oracle, segs, adac.RULE_APPEND, False)
        descs = lay.get_descs()
        assert descs["width"].tolist() == [e[2] for e in enc]
        words = d_words.download(np.uint64, lay.max_arena_words)
        for s, e in enumerate(enc):
            a = int(descs["word_off"][s])
            assert np.array_equal(words[a:a + len(e[4])], e[4]), s
        valid = valid_mask(rng, span, counts, offs)
        info = np.iinfo(dt)
        mid = segs[0][len(segs[0]) // 2]
        probes = [(int(info.min), int(info.max)), (int(min(mid, segs[6][0])), int(max(mid, segs[6][0])))]
        try:
            for cells, templated, per in ((1, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1), (1, 0, 0), (1, 0, 1), (0, 1, 1)):
                adac.set_tuning("scan_cells", cells)
                adac.set_tuning("templated_scan", templated)
                adac.set_tuning("scan_tiles_per_wg", per)
                scan_battery(adac, gpu_ctx, lay, d_words, dt, segs, offs, span, probes, valid,
                             (dt.name, rot, cells, templated, per))
        finally:
            set_knobs(adac, DEFAULT_KNOBS)
    if dt == np.uint8:
        # more than 256 groups with the DEFAULT grouping (4 tiles of u8 per group): 257 * 64 Ki rows
        counts = np.array([257 * 4 * tile - 5, 3, 0, 2 * tile], dtype=np.uint32)
        segs = [make_values(rng, dt, int(c), w) for c, w in zip(counts, (5, 2, 1, 3))]
        lay = adac.Layout(gpu_ctx, dt, counts)
        offs = np.concatenate([[0], np.cumsum(counts[:-1])]).astype(np.int64).tolist()
        span = int(counts.sum())
        d_words = gpu_ctx.alloc(lay.max_arena_words * 8 + 64).zero()
        lay.encode(gpu_ctx.upload(np.concatenate(segs)), d_words, None, adac.RULE_APPEND, False)
        assert lay.get_descs()["width"].tolist() == [e[2] for e in oracle_encode(oracle, segs, adac.RULE_APPEND, False)]
        set_knobs(adac, DEFAULT_KNOBS)
        scan_battery(adac, gpu_ctx, lay, d_words, dt, segs, offs, span, [(0, 255), (3, 17)],
                     valid_mask(rng, span, counts, offs), ("u8 default grouping",))


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_first_come_placement_every_read(adac, oracle, gpu_ctx, dtype):
    """First-come arena placement (encode_placement = 1, the single-pass kernel forced for every type): offsets of the
    encode's own choosing, disjoint and aligned; every read path; then the same values with ordered placement on the
    same layout, every read again, and each segment's words identical between the two placements."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(1_000 + 8 * dt.itemsize + (dt.kind == "i"))
    tile = adac.tile_values(dt)
    counts = [int(x) for x in rng.choice([0, 1, 31, 32, 33, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 5, 15 * tile],
                                         size=90)]
    counts[0] = 15 * tile
    offs, run = [], 0
    for c in counts:
        offs.append(run)
        run += c
    col = Col(adac, gpu_ctx, dt, counts, offs, True)
    try:
        for with_valid in (False, True):
            set_knobs(adac, DEFAULT_KNOBS)
            seed_state = rng.bit_generator.state
            encode_step(adac, oracle, gpu_ctx, col, rng, 2, 1, False, with_valid)
            first = col.lay.get_descs()
            w_first = col.d_words.download(np.uint64, col.nwords)
            check_reads(adac, gpu_ctx, col, rng, ("first-come", with_valid))
            rng.bit_generator.state = seed_state   # the same values, rule and mask again
            encode_step(adac, oracle, gpu_ctx, col, rng, 2, 0, False, with_valid)
            ordered = col.lay.get_descs()
            w_ord = col.d_words.download(np.uint64, col.nwords)
            check_reads(adac, gpu_ctx, col, rng, ("ordered", with_valid))
            for f in ("count", "width", "flags", "min", "val_off"):
                assert np.array_equal(first[f], ordered[f]), f
            for s, e in enumerate(col.enc):
                a, b = int(first["word_off"][s]), int(ordered["word_off"][s])
                assert np.array_equal(w_first[a:a + len(e[4])], w_ord[b:b + len(e[4])]), s
    finally:
        set_knobs(adac, DEFAULT_KNOBS)


def test_context_handle_goes_first_then_its_objects_in_every_order(adac):
    """The context handle is destroyed FIRST, then the layout, the BITPACKING layout, the plan and the event made on it,
    in each of the 24 orders: every object frees its own buffers against the stream that the last of them releases.
    All four have been used, so their lazily made buffers exist (scan groups, arrival cells, the narrow-count words and
    event, both gathers' scratch).  A fresh context decodes 1,000 values after every order."""
    import itertools
    rows = 1000
    vals = ((np.arange(rows, dtype=np.int64) * 2654435761) % 4001).astype(np.int32)
    counts = np.array([rows], dtype=np.uint32)
    sel = np.arange(1024) % 2 == 0
    sel[rows:] = False
    bitmap = np.packbits(sel, bitorder="little").view(np.uint64)
    for order in itertools.permutations(range(4)):
        ctx = adac.Context(0)
        d_vals, d_bitmap = ctx.upload(vals), ctx.upload(bitmap)
        d_out, d_sum = ctx.alloc(rows * 4 + 16), ctx.alloc(8)
        lay = adac.Layout(ctx, np.int32, counts)
        d_words = ctx.alloc(lay.max_arena_words * 8 + 16).zero()
        lay.encode(d_vals, d_words)
        lay.scan_sum(d_words, d_sum)
        assert lay.unpack_selected(d_words, d_bitmap, d_out) == rows // 2
        assert int(d_sum.download(np.uint64, 1)[0]) == int(vals.sum())
        plan = adac.BitpackingPlan(ctx, np.int32, d_vals, rows)
        d_blocks = ctx.alloc(plan.nseg * plan.BLOCK_STRIDE + 64)
        plan.write(d_vals, d_blocks)
        bp = adac.BitpackingLayout(ctx, np.int32, np.arange(plan.nseg, dtype=np.uint64) * plan.BLOCK_STRIDE,
                                   [plan.segment(i)[1] for i in range(plan.nseg)])
        assert bp.unpack_selected(d_blocks, d_bitmap, d_out) == rows // 2
        ev = adac.Event(ctx)
        ev.wait()
        ctx.close()   # frees the raw buffers; the C context lives on in the four objects
        objs = [lay, bp, plan, ev]
        for i in order:
            objs[i].close()
        ctx2 = adac.Context(0)
        lay2 = adac.Layout(ctx2, np.int32, counts)
        d2, out2 = ctx2.upload(vals), ctx2.alloc(rows * 4 + 16)
        w2 = ctx2.alloc(lay2.max_arena_words * 8 + 16).zero()
        lay2.encode(d2, w2)
        lay2.unpack(w2, out2)
        assert np.array_equal(out2.download(np.int32, rows), vals), order
        lay2.close()
        ctx2.close()
