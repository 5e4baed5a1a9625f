"""The cells of tests/test_gpu_big_segment_scans.py: the scan families that came after test_gpu_big_segments.py, each on
a segment just below and a segment at (or past) 2^31 / 2^32 bits, where its register walk hands over to its staged
reader.  tests/test_big_scan_census.py states on the CPU, from numpy's min / max and the width rule alone, what every
cell relies on; the GPU file makes the same statements on the device's own descriptors before it launches anything.

A cell names the big column (test_gpu_big_segments.COLUMNS, or the dense key column k16 below), the role it plays, and
one maker per partner role.  Partners are as narrow and as small a type as the role allows (u8 keys below 6, u16 at
w <= 10), except where the role forces more: `a` of the product rules and the key of the walk readers are at least 4
bits wide, a compare partner has the big column's type because its frame must lie inside the big column's (else the
headers decide every row), and side b of the past-2^32 compare cell is a u64 column of w 63 itself.

k16 (uint16, w 15, frame 1000): rows_below(2^31, 15) and rows_reaching(2^31, 15) rows and 4097 rows at w 9.  The u32
column's keys span 2^31 values, so a domain of any size a test can afford holds almost none of its rows; k16's full
domain is 2^15 keys and holds every row.  The keys at threshold_rows() of the two big segments and at their last rows
are overwritten with values inside K16_WINDOW, the smallest domain used, which K16_SLICE contains: the narrow-domain
cells have in-domain rows exactly where the arithmetic is at its limit.  (The last row of the small segment holds its
frame's top value, 1511, which lies in both narrow domains as it is.)

Every expectation is numpy over the raw values: uint64 wrapping products and sums (np.add.at on uint64, or the family
files' per-group sums), np.bincount for the dense counts, np.packbits for bitmaps, np.unique for the built set."""
import importlib

import numpy as np

import scan_compare_cases as sc
import scan_member_cases as sm
from scan_member_cases import kind
from test_gpu_big_segments import (B31, B32, column_from, hashed, make_column, mask_words, memset, rows_below,
                                   rows_reaching, small_keys, threshold_rows)
from test_gpu_group_sum import reference_groups
from test_gpu_group_sum_product import reference as reference_product
from test_gpu_group_sum_product3 import reference as reference_product3
from test_gpu_group_sum_q1 import TERMS, reference_q1
from test_gpu_sum_product import widen

forms = importlib.import_module("duckdb-adaptive-compression_amd.forms")

POISON_BYTE, POISON = 0xEE, 0xEEEEEEEEEEEEEEEE
NGROUPS = 6
RW_KNOBS = ("group_sum_rw", "group_product_rw", "group_product3_rw", "group_q1_rw")

K16_BASE = 1000
K16 = (np.uint16, [(rows_below(B31, 15), 15, K16_BASE), (rows_reaching(B31, 15), 15, K16_BASE), (4097, 9, K16_BASE)])
K16_FULL = (K16_BASE, 1 << 15)
K16_WINDOW = (K16_BASE + 200, forms.DENSE_WINDOW)     # the smallest domain: the planted keys lie inside
K16_SLICE = (K16_BASE + 100, forms.MAPPED_SLICE)      # holds K16_WINDOW
KEY7 = (0, 128)                                       # the domain of the u8 key column of w 7


def planted_rows(c):
    """(element index, segment) of the rows of the big segments where the arithmetic is at its limit"""
    out = []
    for s in c.big:
        n = int(c.counts[s])
        out += [(c.offs[s] + r, s) for r in sorted(set(threshold_rows(n, c.widths[s]) + [n - 1]))]
    return out


def make_k16():
    c = column_from("k16", K16[0], K16[1], (0, 1))
    for j, (e, _) in enumerate(planted_rows(c)):
        c.vals[e] = K16_WINDOW[0] + 1 + (37 * j) % (K16_WINDOW[1] - 2)
    c.minmax = [(int(v.min()), int(v.max())) for v in c.segs]
    return c


def big_column(name):
    return make_k16() if name == "k16" else make_column(name)


# ---------------------------------------------------------------------------------------------------------------------
# partner columns, by role; each a function of the big column alone
# ---------------------------------------------------------------------------------------------------------------------
def code_of(keys):
    """the group code of a key VALUE (a function of the key, so a built map has one answer): 0 ... 8, NGROUPS is 6"""
    return ((keys.astype(np.uint32) * np.uint32(7) + np.uint32(3)) % np.uint32(9)).astype(np.uint8)


def map_for(domain):
    base, span = domain
    return code_of(np.arange(base, base + span, dtype=np.uint32))


def overlapping(c, bits, salt):
    """A column of c's type and counts whose frame lies INSIDE c's in every segment, so that no segment pair is decided
    by the two headers; `bits` wide (less where c's segment is narrower).  Where c's own value falls into that frame the
    partner takes it: those are CMP_EQ's rows."""
    out = np.empty(c.n, dtype=c.dtype)
    for s, (v, o) in enumerate(zip(c.segs, c.offs)):
        mn, mx = c.minmax[s]
        b = min(bits, c.widths[s] - 1)
        base = mn + (mx - mn) // 4
        assert base + 2 ** b - 1 <= mx
        p = hashed(len(v), b, base, c.dtype, salt=salt + s)
        same = (v >= c.dtype.type(base)) & (v <= c.dtype.type(base + 2 ** b - 1))
        p[same] = v[same]
        out[o:o + len(v)] = p
    return out


def overlapping_full(c, salt):
    """A column of c's type, counts, widths and frames from another stretch of the hash; equal to c at every 997th row and
    at the threshold rows of the big segments."""
    out = np.empty(c.n, dtype=c.dtype)
    for s, (v, o) in enumerate(zip(c.segs, c.offs)):
        out[o:o + len(v)] = hashed(len(v), c.widths[s], c.minmax[s][0], c.dtype, salt=salt + s)
    out[::997] = c.vals[::997]
    for e, _ in planted_rows(c):
        out[e] = c.vals[e]
    return out


PARTNERS = {
    "keys": lambda c: small_keys(c.n, NGROUPS),                          # u8, w 3
    "a": lambda c: hashed(c.n, 9, 50, np.uint16, salt=17),               # the product rules want w >= 4 of a
    "b": lambda c: hashed(c.n, 5, 1000, np.uint16, salt=7),
    "c": lambda c: hashed(c.n, 7, 3, np.uint16, salt=11),
    "q": lambda c: hashed(c.n, 6, 1, np.uint16, salt=13),
    "values": lambda c: hashed(c.n, 10, 7, np.uint16, salt=3),
    "key7": lambda c: hashed(c.n, 7, 0, np.uint8, salt=19),              # a dense key the walk readers take (w >= 4)
    "codes": lambda c: code_of(c.vals),                                  # of the key column itself
    "near10": lambda c: overlapping(c, 10, 29),
    "near3": lambda c: overlapping(c, 3, 31),
    "twin": lambda c: overlapping_full(c, 37),
}
BIG = "the big column"


# ---------------------------------------------------------------------------------------------------------------------
# descriptors and forms
# ---------------------------------------------------------------------------------------------------------------------
def expected_descs(width_of, vals, counts):
    """What the encode must produce, from numpy's min / max and the width rule (unsigned columns, every segment packed)."""
    tb = 8 * vals.dtype.itemsize
    out, pos = [], 0
    for n in counts:
        v = vals[pos:pos + int(n)]
        pos += int(n)
        mn, mx = int(v.min()), int(v.max())
        w = width_of(mn, mx)
        assert vals.dtype.kind == "u" and 0 < w < tb
        out.append({"count": int(n), "width": w, "min": mn, "flags": 1})
    return out


def group_forms(value_descs, kinds, descs_k):
    """forms.form_groups segment by segment -> "fast" / "generic" per segment"""
    out = []
    for s in range(len(descs_k)):
        f = forms.form_groups(tuple([d[s]] for d in value_descs), kinds, [descs_k[s]], NGROUPS, 1)
        assert (f["fast"] == 0) != (f["generic"] == 0)
        out.append("fast" if f["fast"] else "generic")
    return out


def generic_scan_groups(value_descs, kinds, descs_k):
    """what the register walk must leave to the staged kernel: adac_debug_group_handover's word"""
    return forms.form_groups(tuple(value_descs), kinds, descs_k, NGROUPS, 1)["generic"]


class Cell:
    """family / name: the row and the cell of the matrix; column: the big column; roles: ((role, BIG or a key of
    PARTNERS), ...) in the order the rule reads them; forms(d, k): the forms per segment from the descriptors d[role] and
    the types k[role]; want: what they must be; run: the GPU side; mask: the salt of mask_words, where the cell has a
    validity mask; domain: (base, span) of the dense cells; variants: which of "no mask" and "mask" a cell of a family
    that runs both takes (a cell is split where both together would take too long)."""

    def __init__(self, family, name, column, roles, forms, want, run, mask=None, domain=None, knob=None,
                 variants=("no mask", "mask")):
        self.family, self.name, self.column, self.roles, self.forms, self.want = family, name, column, roles, forms, want
        self.run, self.domain, self.knob, self.variants = run, domain, knob, variants
        self.mask = mask if "mask" in variants else None
        self.id = "%s-%s" % (column, name)

    def partner_values(self, c, cache=None):
        """role -> raw values"""
        cache = {} if cache is None else cache
        out = {}
        for role, maker in self.roles:
            if maker is BIG:
                out[role] = c.vals
            else:
                if maker not in cache:
                    cache[maker] = PARTNERS[maker](c)
                out[role] = cache[maker]
        return out

    def check_forms(self, descs, kinds, where):
        got = self.forms(descs, kinds)
        assert got == self.want, (self.family, self.id, where, got, self.want)


def statement(cell, got, want, what):
    assert got == want, (cell.family, cell.id, what, got, want)


# ---------------------------------------------------------------------------------------------------------------------
# the GPU side
# ---------------------------------------------------------------------------------------------------------------------
class Side:
    """one column of a scan: raw values, layout, packed words, the device's descriptors"""

    def __init__(self, vals, lay, words, descs, owned):
        self.vals, self.lay, self.words, self.descs, self.owned = vals, lay, words, descs, owned
        self.kind = kind(vals.dtype)

    def free(self):
        if self.owned:
            self.lay.close()
            self.words.free()


class Env:
    def __init__(self, adac, ctx):
        self.adac, self.ctx = adac, ctx

    def encode(self, vals, counts):
        lay = self.adac.Layout(self.ctx, vals.dtype, counts)
        assert lay.value_span == len(vals)
        d_vals = self.ctx.upload(vals)
        words = self.ctx.alloc(lay.max_arena_words * 8 + 16).zero()
        lay.encode(d_vals, words)
        self.ctx.sync()
        d_vals.free()
        return Side(vals, lay, words, lay.get_descs(), True)

    def out(self, nwords):
        """an output of nwords words and a spare one"""
        return (self.ctx.alloc((nwords + 1) * 8), nwords)

    def call(self, outs, launch):
        """every output poisoned, the launch, every output read back; the spare word must keep the poison"""
        for buf, _ in outs:
            memset(self.adac, self.ctx, buf, POISON_BYTE)
        launch()
        got = []
        for buf, n in outs:
            w = buf.download(np.uint64, n + 1)
            assert int(w[n]) == POISON, "a word past the result was written"
            got.append(w[:n])
        return got

    def mask(self, c, salt):
        """(device words, bool per row) of the cell's validity mask; (None, None) without one"""
        if salt is None:
            return None, None
        words, keep = mask_words(c.n, salt)
        return self.ctx.upload(words), keep


def run_cell(adac, ctx, c, cell):
    """Encode the partners, state the forms on the device's descriptors, run the cell, free the partners."""
    env = Env(adac, ctx)
    vals = cell.partner_values(c)
    sides = {}
    try:
        for role, maker in cell.roles:
            sides[role] = Side(c.vals, c.lay, c.d_words, c.descs, False) if maker is BIG else env.encode(vals[role], c.counts)
        cell.check_forms({r: s.descs for r, s in sides.items()}, {r: s.kind for r, s in sides.items()}, "device")
        cell.run(env, c, sides, cell)
    finally:
        for s in sides.values():
            s.free()


def rows_per_segment(mask, c):
    return [int(np.count_nonzero(mask[o:o + int(n)])) for o, n in zip(c.offs, c.counts)]


def same_words(got, exp, cell, what):
    wrong = np.flatnonzero(got != exp)
    assert len(wrong) == 0, (cell.family, cell.id, what, len(wrong), [(int(i), int(got[i]), int(exp[i])) for i in wrong[:4]])


def same_bitmap(words, hit, cell, what):
    """every byte of the bitmap: np.packbits of the hits, zero from there to the last word"""
    exp = np.packbits(hit, bitorder="little")
    got = words.view(np.uint8)
    if not (np.array_equal(got[:len(exp)], exp) and not got[len(exp):].any()):
        bad = np.flatnonzero(got[:len(exp)] != exp)
        raise AssertionError((cell.family, cell.id, what, bad[:4].tolist(), len(bad), int(got[len(exp):].any())))


# ---- the four register-walk families: knob at 1, 0, 1 ---------------------------------------------------------------
def grouped_runs(env, c, cell, lead, values, keys, out_words, launch, variants):
    """launch(outs, d_mask) with the cell's knob at 1, 0 and 1 again, for every (what, d_mask, expected word lists) of
    `variants`: every word against numpy, and the hand-over word against forms.py."""
    generic = generic_scan_groups([s.descs for s in values], [s.kind for s in values], keys.descs)
    outs = [env.out(n) for n in out_words]
    try:
        for what, d_mask, exp in variants:
            for rw in (1, 0, 1):
                env.adac.set_tuning(cell.knob, rw)
                got = env.call(outs, lambda: launch([b for b, _ in outs], d_mask))
                for g, e in zip(got, exp):
                    statement(cell, g.tolist(), list(e), (what, "knob", rw))
                statement(cell, lead.lay.debug_group_handover(), generic if rw else 0, (what, "hand-over", rw))
    finally:
        env.adac.set_tuning(cell.knob, 1)
        for b, _ in outs:
            b.free()


def masked_and_not(env, c, cell):
    """[(what, bool per row or None, the mask's buffer or None)] for the cell's variants; -> (them, the mask's buffer)"""
    d_mask, keep = env.mask(c, cell.mask)
    both = {"no mask": ("no mask", None, None), "mask": ("mask", keep, d_mask)}
    return [both[v] for v in cell.variants], d_mask


def release(*bufs):
    for buf in bufs:
        if buf is not None:
            buf.free()


def in_chunks(n, part, step=1 << 20):
    """part(rows lo ... hi as a slice) -> per-bin uint64 sums of those rows; added up mod 2^64 over the column, so that a
    reference's temporaries stay a few MiB"""
    acc = None
    for lo in range(0, n, step):
        r = np.array(part(slice(lo, min(n, lo + step))), dtype=np.uint64)
        acc = r if acc is None else acc + r
    return acc


def run_group_sum_valid(env, c, S, cell):
    v, k = S["value"], S["keys"]
    d_mask, keep = env.mask(c, cell.mask)
    exp = reference_groups(v.vals[keep], k.vals[keep], NGROUPS)
    grouped_runs(env, c, cell, v, [v], k, [NGROUPS + 1] * 2,
                 lambda o, m: v.lay.scan_group_sum_valid(v.words, k.lay, k.words, m, NGROUPS, o[0], o[1]),
                 [("mask", d_mask, exp)])
    d_mask.free()


def run_group_sum_product(env, c, S, cell):
    a, b, k = S["a"], S["b"], S["keys"]
    variants, d_mask = masked_and_not(env, c, cell)
    variants = [(what, d_m, reference_product(a.vals, b.vals, k.vals, NGROUPS, keep)) for what, keep, d_m in variants]
    grouped_runs(env, c, cell, a, [a, b], k, [NGROUPS + 1] * 2,
                 lambda o, m: a.lay.scan_group_sum_product(a.words, b.lay, b.words, k.lay, k.words, NGROUPS, o[0], o[1], m),
                 variants)
    release(d_mask)


def run_group_sum_product3(env, c, S, cell):
    a, b, cc, k = S["a"], S["b"], S["c"], S["keys"]
    variants, d_mask = masked_and_not(env, c, cell)
    variants = [(what, d_m, reference_product3(a.vals, b.vals, cc.vals, k.vals, NGROUPS, keep)) for what, keep, d_m in variants]
    grouped_runs(env, c, cell, a, [a, b, cc], k, [NGROUPS + 1] * 2,
                 lambda o, m: a.lay.scan_group_sum_product3(a.words, b.lay, b.words, cc.lay, cc.words, k.lay, k.words,
                                                            NGROUPS, o[0], o[1], m), variants)
    release(d_mask)


def run_group_sum_q1(env, c, S, cell):
    a, b, cc, q, k = S["a"], S["b"], S["c"], S["q"], S["keys"]
    variants, d_mask = masked_and_not(env, c, cell)

    def reference(keep):
        terms = in_chunks(c.n, lambda rows: reference_q1(a.vals[rows], b.vals[rows], cc.vals[rows], q.vals[rows],
                                                        k.vals[rows], NGROUPS, None if keep is None else keep[rows]))
        return [terms.reshape(-1).tolist()]
    variants = [(what, d_m, reference(keep)) for what, keep, d_m in variants]
    grouped_runs(env, c, cell, a, [a, b, cc, q], k, [TERMS * (NGROUPS + 1)],
                 lambda o, m: a.lay.scan_group_sum_q1(a.words, b.lay, b.words, cc.lay, cc.words, q.lay, q.words, k.lay,
                                                      k.words, NGROUPS, o[0], m), variants)
    release(d_mask)


# ---- the compare scans ----------------------------------------------------------------------------------------------
COMPARE_CMPS = (sc.LT, sc.EQ)


def run_compare(env, c, S, cell):
    a, b = S["a"], S["b"]
    masks = sc.compare_masks(a.vals, b.vals)
    variants, d_mask = masked_and_not(env, c, cell)
    nseg, nw = len(c.counts), (c.n + 63) // 64
    bm, cnt = env.out(nw), env.out(nseg)
    for what, k_, d_m in variants:
        for cmp in COMPARE_CMPS:
            hit = sc.hits_of(masks, cmp, k_)
            exp_cnt = rows_per_segment(hit, c)
            got_bm, got_cnt = env.call([bm, cnt], lambda: a.lay.scan_select_compare(a.words, b.lay, b.words, cmp, bm[0],
                                                                                     cnt[0], d_m))
            statement(cell, got_cnt.tolist(), exp_cnt, (what, cmp, "select's counts"))
            same_bitmap(got_bm, hit, cell, (what, cmp))
            (got_cnt,) = env.call([cnt], lambda: a.lay.scan_count_compare(a.words, b.lay, b.words, cmp, cnt[0], d_m))
            statement(cell, got_cnt.tolist(), exp_cnt, (what, cmp, "count form"))
            del hit, got_bm
    release(bm[0], cnt[0], d_mask)


# ---- the member scans -----------------------------------------------------------------------------------------------
def member_set(bits):
    """a set over `bits` values, about half of them members"""
    return mask_words(bits, 23)[0][:sm.set_words_for(bits)].copy()


def sparse_keep(c):
    """a mask that keeps few rows: the 3000 rows up to and the row after every planted row, and every 4099th row"""
    keep = np.zeros(c.n, dtype=bool)
    keep[::4099] = True
    for e, s in planted_rows(c):
        keep[max(c.offs[s], e - 3000):min(c.offs[s] + int(c.counts[s]), e + 2)] = True
    return keep


def keep_words(keep):
    """bool per element -> the mask's u64 words and a spare one"""
    nw = (len(keep) + 63) // 64
    full = np.zeros(nw * 64, dtype=bool)
    full[:len(keep)] = keep
    return np.concatenate([np.packbits(full, bitorder="little").view(np.uint64), np.zeros(1, dtype=np.uint64)])


def built_set(vals, base, bits):
    """the set a build over `vals` must leave: np.unique of the values inside the domain"""
    u = np.unique(vals).astype(np.int64) - base
    u = u[(u >= 0) & (u < bits)]
    member = np.zeros(sm.set_words_for(bits) * 64, dtype=bool)
    member[u] = True
    return np.packbits(member, bitorder="little").view(np.uint64)


def run_member(env, c, S, cell):
    col = S["column"]
    base, bits = cell.domain
    nseg, nw, nset = len(c.counts), (c.n + 63) // 64, sm.set_words_for(bits)
    cnt = env.out(nseg)
    if cell.name == "build":
        built = env.out(nset)
        sparse = sparse_keep(c)
        d_sparse = env.ctx.upload(keep_words(sparse))
        _, inside = sm.member_index(col.vals, base, bits)
        for what, k_, d_m in (("no mask", None, None), ("sparse mask", sparse, d_sparse)):
            wanted = col.vals if k_ is None else col.vals[k_]
            exp_cnt = rows_per_segment(inside if k_ is None else inside & k_, c)
            got_set, got_cnt = env.call([built, cnt], lambda: col.lay.scan_build_member(col.words, base, bits, built[0],
                                                                                        cnt[0], d_m))
            statement(cell, got_cnt.tolist(), exp_cnt, (what, "rows in the domain"))
            same_words(got_set, built_set(wanted, base, bits), cell, what)
        release(built[0], d_sparse, cnt[0])
        return
    set_words = member_set(bits)
    d_set = env.ctx.upload(set_words)
    variants, d_mask = masked_and_not(env, c, cell)
    bm = env.out(nw)
    for what, k_, d_m in variants:
        hit = sm.member_mask(col.vals, base, bits, set_words, k_)
        exp_cnt = rows_per_segment(hit, c)
        got_bm, got_cnt = env.call([bm, cnt], lambda: col.lay.scan_select_member(col.words, d_set, base, bits, bm[0], cnt[0],
                                                                                 d_m))
        statement(cell, got_cnt.tolist(), exp_cnt, (what, "select's counts"))
        same_bitmap(got_bm, hit, cell, what)
        (got_cnt,) = env.call([cnt], lambda: col.lay.scan_count_member(col.words, d_set, base, bits, cnt[0], d_m))
        statement(cell, got_cnt.tolist(), exp_cnt, (what, "count form"))
        del hit, got_bm
    release(bm[0], cnt[0], d_set, d_mask)


# ---- the dense-key scans and the scans through a map ----------------------------------------------------------------
def indexed(keys, domain, keep):
    """(index of every wanted row inside the domain, which rows those are)"""
    t, inside = sm.member_index(keys, domain[0], domain[1])
    if keep is not None:
        inside &= keep
    return t[inside].astype(np.int64), inside


def summed(idx, terms, nbins):
    """per bin: the sum mod 2^64 of every term (uint64 per wanted row), and the rows (np.bincount)"""
    sums = []
    for t in terms:
        acc = np.zeros(nbins, dtype=np.uint64)
        np.add.at(acc, idx, t)
        sums.append(acc)
    return sums, np.bincount(idx, minlength=nbins).astype(np.uint64)


def run_dense(env, c, S, cell):
    k, v = S["key"], S["value"]
    base, span = cell.domain
    nseg = len(c.counts)
    d_mask, keep = env.mask(c, cell.mask)
    idx, inside = indexed(k.vals, cell.domain, keep)
    (exp_s,), exp_c = summed(idx, [widen(v.vals)[inside]], span)
    exp_r = rows_per_segment(inside, c)
    del idx
    sums, counts, rows = env.out(span), env.out(span), env.out(nseg)
    got_s, got_c, got_r = env.call([sums, counts, rows], lambda: k.lay.scan_group_sum_dense(
        k.words, v.lay, v.words, base, span, sums[0], counts[0], rows[0], d_mask))
    same_words(got_s, exp_s, cell, "sums")
    same_words(got_c, exp_c, cell, "counts")
    statement(cell, got_r.tolist(), exp_r, "rows per segment")
    got_c, got_r = env.call([counts, rows], lambda: k.lay.scan_group_count_dense(k.words, base, span, counts[0], rows[0],
                                                                                 d_mask))
    same_words(got_c, exp_c, cell, "count entry")
    statement(cell, got_r.tolist(), exp_r, "count entry, rows per segment")
    for buf in (sums[0], counts[0], rows[0], d_mask):
        if buf is not None:
            buf.free()


def map_words(codes, pad=0xA5):
    """span codes -> the map's allocation (a multiple of 8 bytes, its pad bytes set to `pad`) as words"""
    out = np.full((len(codes) + 7) // 8 * 8, pad, dtype=np.uint8)
    out[:len(codes)] = codes
    return out.view(np.uint64)


def run_mapped(env, c, S, cell):
    k, v = S["key"], S["value"]
    base, span = cell.domain
    nseg, nb = len(c.counts), NGROUPS + 1
    d_mask, keep = env.mask(c, cell.mask)
    rows = env.out(nseg)
    if "codes" in S:
        # the build: every byte of the map against numpy; codes are a function of the key, so every index has one answer
        codes = S["codes"]
        idx, inside = indexed(k.vals, cell.domain, keep)
        exp_map = np.full((span + 7) // 8 * 8, 255, dtype=np.uint8)
        exp_map[idx] = codes.vals[inside]
        exp_r = rows_per_segment(inside, c)
        del idx, inside
        built = env.out(len(exp_map) // 8)
        got_map, got_r = env.call([built, rows], lambda: k.lay.scan_build_map(k.words, codes.lay, codes.words, base, span,
                                                                              built[0], 255, rows[0], d_mask))
        same_words(got_map.view(np.uint8), exp_map, cell, "every byte of the built map")
        statement(cell, got_r.tolist(), exp_r, "build, rows per segment")
        assert np.array_equal(exp_map[:span], map_for(cell.domain))    # the map the other cells go through
        release(built[0], rows[0], d_mask)
        return
    d_map = env.ctx.upload(map_words(map_for(cell.domain)))
    idx, inside = indexed(k.vals, cell.domain, keep)
    g = np.minimum(map_for(cell.domain)[idx], NGROUPS).astype(np.int64)
    (exp_s,), exp_c = summed(g, [widen(v.vals)[inside]], nb)
    exp_r = rows_per_segment(inside, c)
    del idx, g
    sums, counts = env.out(nb), env.out(nb)
    got_s, got_c, got_r = env.call([sums, counts, rows], lambda: k.lay.scan_group_sum_mapped(
        k.words, v.lay, v.words, d_map, base, span, NGROUPS, sums[0], counts[0], rows[0], d_mask))
    same_words(got_s, exp_s, cell, "sums")
    same_words(got_c, exp_c, cell, "counts")
    statement(cell, got_r.tolist(), exp_r, "rows per segment")
    got_c, got_r = env.call([counts, rows], lambda: k.lay.scan_group_count_mapped(k.words, d_map, base, span, NGROUPS,
                                                                                  counts[0], rows[0], d_mask))
    same_words(got_c, exp_c, cell, "count entry")
    statement(cell, got_r.tolist(), exp_r, "count entry, rows per segment")
    for buf in (sums[0], counts[0], rows[0], d_map, d_mask):
        if buf is not None:
            buf.free()


def run_product_mapped(env, c, S, cell):
    k, a, b = S["key"], S["a"], S["b"]
    base, span = cell.domain
    nseg, nb = len(c.counts), NGROUPS + 1
    d_mask, keep = env.mask(c, cell.mask)
    d_map = env.ctx.upload(map_words(map_for(cell.domain)))
    codes, inside = map_for(cell.domain), np.empty(c.n, dtype=bool)

    def part(rows):
        idx, inside[rows] = indexed(k.vals[rows], cell.domain, None if keep is None else keep[rows])
        g = np.minimum(codes[idx], NGROUPS).astype(np.int64)
        wa, wb = widen(a.vals[rows])[inside[rows]], widen(b.vals[rows])[inside[rows]]
        (ab, sa), cn = summed(g, [wa * wb, wa], nb)
        return [ab, sa, cn]
    exp_ab, exp_a, exp_c = in_chunks(c.n, part)
    exp_r = rows_per_segment(inside, c)
    outs = [env.out(nb), env.out(nb), env.out(nb), env.out(nseg)]
    got_ab, got_a, got_c, got_r = env.call(outs, lambda: k.lay.scan_group_sum_product_mapped(
        k.words, a.lay, a.words, b.lay, b.words, d_map, base, span, NGROUPS, outs[0][0], outs[1][0], outs[2][0],
        outs[3][0], d_mask))
    same_words(got_ab, exp_ab, cell, "sums of a * b")
    same_words(got_a, exp_a, cell, "sums of a")
    same_words(got_c, exp_c, cell, "counts")
    statement(cell, got_r.tolist(), exp_r, "rows per segment")
    for buf in [o[0] for o in outs] + [d_map, d_mask]:
        if buf is not None:
            buf.free()


# ---------------------------------------------------------------------------------------------------------------------
# the matrix
# ---------------------------------------------------------------------------------------------------------------------
def grouped(family, knob, run, name, column, roles, want, variants, mask=11):
    values = [r for r, _ in roles if r != "keys"]
    return [Cell(family, name + ("-masked" if v == "mask" and len(variants) > 1 else ""), column, roles,
                 lambda d, k: group_forms([d[r] for r in values], [k[r] for r in values], d["keys"]), want, run, mask, None,
                 knob, (v,)) for v in variants]


def compare(name, column, roles, want):
    return Cell("compare", name, column, roles,
                lambda d, k: forms.compare_form_groups(d["a"], d["b"], k["a"], k["b"]), want, run_compare, 13)


def member(name, column, domain, want, variants, mask=15):
    return [Cell("member", name + ("-masked" if v == "mask" else ""), column, (("column", BIG),),
                 lambda d, k: forms.member_form_groups(d["column"], k["column"], *domain), want, run_member, mask, domain,
                 None, (v,)) for v in variants]


def dense(name, column, roles, domain, want, mask=None):
    return Cell("dense", name, column, roles,
                lambda d, k: forms.dense_form_groups(d["key"], k["key"], domain[0], domain[1], d["value"], k["value"]),
                want, run_dense, mask, domain)


def mapped(name, column, roles, domain, want, mask=None):
    reads = "codes" if any(r == "codes" for r, _ in roles) else None

    def both(d, k):
        f = forms.mapped_form_groups(d["key"], k["key"], domain[0], domain[1], d["value"], k["value"])
        if reads:   # the build reads the codes where the sum reads the values: the same forms
            assert f == forms.mapped_form_groups(d["key"], k["key"], domain[0], domain[1], d[reads], k[reads])
        return f
    return Cell("mapped", name, column, roles, both, want, run_mapped, mask, domain)


def product_mapped(name, column, roles, domain, want, mask=None):
    return Cell("product_mapped", name, column, roles,
                lambda d, k: forms.mapped_product_form_groups(d["key"], k["key"], domain[0], domain[1], d["a"], k["a"],
                                                              d["b"], k["b"]), want, run_product_mapped, mask, domain)


BELOW_AT_SMALL = ["fast", "generic", "fast"]        # u32: S0 below the gate, S1 at it, the small S2
ALL_GENERIC = ["generic"] * 3                       # u64: w 63 / 63 / 40, past 2^32 bits
K, A, B, C_, Q = ("keys", "keys"), ("a", "a"), ("b", "b"), ("c", "c"), ("q", "q")

BOTH, MASKED, UNMASKED = ("no mask", "mask"), ("mask",), ("no mask",)
K16_MEMBER = ["walk-slice", "staged-slice", "walk-slice"]

CELLS = [
    *grouped("group_sum_valid", "group_sum_rw", run_group_sum_valid, "value", "u32", (("value", BIG), K), BELOW_AT_SMALL,
             MASKED, 5),
    *grouped("group_sum_product", "group_product_rw", run_group_sum_product, "a", "u32", (("a", BIG), B, K), BELOW_AT_SMALL,
             BOTH),
    *grouped("group_sum_product", "group_product_rw", run_group_sum_product, "b", "u32", (A, ("b", BIG), K), BELOW_AT_SMALL,
             BOTH),
    *grouped("group_sum_product", "group_product_rw", run_group_sum_product, "a", "u64", (("a", BIG), B, K), ALL_GENERIC,
             BOTH),
    *grouped("group_sum_product3", "group_product3_rw", run_group_sum_product3, "c", "u32", (A, B, ("c", BIG), K),
             BELOW_AT_SMALL, UNMASKED),
    *grouped("group_sum_q1", "group_q1_rw", run_group_sum_q1, "q", "u32", (A, B, C_, ("q", BIG), K), BELOW_AT_SMALL,
             UNMASKED),
    *grouped("group_sum_q1", "group_q1_rw", run_group_sum_q1, "a", "u32", (("a", BIG), B, C_, Q, K), BELOW_AT_SMALL,
             UNMASKED),
    compare("a", "u32", (("a", BIG), ("b", "near10")), BELOW_AT_SMALL),
    compare("b", "u32", (("a", "near10"), ("b", BIG)), BELOW_AT_SMALL),
    compare("a", "u64", (("a", BIG), ("b", "twin")), ALL_GENERIC),
    compare("a", "u8", (("a", BIG), ("b", "near3")), ["generic", "generic"]),
    *member("select-count", "k16", K16_FULL, K16_MEMBER, BOTH),
    *member("build", "k16", K16_FULL, K16_MEMBER, UNMASKED),
    *member("select-count", "u8", (100, 128), ["staged-slice", "staged-slice"], BOTH),
    dense("key-full", "k16", (("key", BIG), ("value", "values")), K16_FULL, ["walk-direct", "staged-direct", "walk-window"]),
    dense("key-window", "k16", (("key", BIG), ("value", "values")), K16_WINDOW,
          ["walk-window", "staged-window", "walk-window"], 7),
    dense("value", "u32", (("key", "key7"), ("value", BIG)), KEY7, ["walk-window", "staged-window", "walk-window"], 9),
    dense("value", "u64", (("key", "key7"), ("value", BIG)), KEY7, ["staged-window"] * 3),
    mapped("key-full-build", "k16", (("key", BIG), ("codes", "codes"), ("value", "values")), K16_FULL,
           ["walk-direct", "staged-direct", "walk-slice"]),
    mapped("key-full", "k16", (("key", BIG), ("value", "values")), K16_FULL, ["walk-direct", "staged-direct", "walk-slice"]),
    mapped("key-slice", "k16", (("key", BIG), ("value", "values")), K16_SLICE, ["walk-slice", "staged-slice", "walk-slice"],
           7),
    product_mapped("key-full", "k16", (("key", BIG), A, B), K16_FULL, ["walk-direct", "staged-direct", "walk-slice"]),
    product_mapped("a", "u32", (("key", "key7"), ("a", BIG), B), KEY7, ["walk-slice", "staged-slice", "walk-slice"], 9),
    product_mapped("b", "u32", (("key", "key7"), A, ("b", BIG)), KEY7, ["walk-slice", "staged-slice", "walk-slice"]),
    product_mapped("a", "u64", (("key", "key7"), ("a", BIG), B), KEY7, ["staged-slice"] * 3),
]
FAMILIES = ("group_sum_valid", "group_sum_product", "group_sum_product3", "group_sum_q1", "compare", "member", "dense",
            "mapped", "product_mapped")
BIG_COLUMNS = ("u32", "u64", "u8", "k16")


def cells_of(family=None, column=None):
    return [x for x in CELLS if family in (None, x.family) and column in (None, x.column)]
