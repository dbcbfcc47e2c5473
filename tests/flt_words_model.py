"""A numpy model of the filter scans' tile word (csrc/rr_x3.h: rr_flt_gap_code / rr_flt_gap_steps, csrc/rr_dense_flt.hip:
the epilogues of rr_scan_flt, rr_scan_flt16, rr_scan_fltq) and check_words(), which holds a scan's raw output against a
float64 reference.  Used by test_flt_words_model.py (CPU: the model against itself, with teeth) and by
test_gpu_flt_words.py (the kernels against the model).

The word of (32-row tile, query):  low half  = the tile's maximum filter score as bf16, rounded UP;
                                   high half = four 4-bit codes, one per 8-row M-tile g: how far the M-tile's maximum sits
below the tile's, in units of step = (smallest finite positive eps of the launch) / 2, rounded DOWN on a two-slope scale
(codes 0..7: one step each, 8..15: two steps each from 8 steps on, 15 = "22 steps or more").  The decoded bound
mx - steps(code) * step is an upper bound of the M-tile's maximum.

What check_words() asks (M8 = float64 maximum of sum_k bf16(a_k) bf16(q_k) over the REAL rows of an 8-row M-tile, -inf
where it has none; delta = gamma_384 * max over those rows of sum_k |bf16(a_k) bf16(q_k)|: the worst case of any fp32
summation order, so every scan's own m8 lies in [M8 - delta, M8 + delta]; M32 - delta := max_g (M8_g - delta_g), M32 + delta
likewise):

  P1 safe maximum    mx >= M32 - delta
  P2 safe gaps       mx - steps(code_g) step >= M8_g - delta_g
  P3 tight maximum   mx <= bf16_up(M32 + delta)
  P4 tight gaps      mx - steps(code_g) step <= M8_g + slack_g, or code_g = 15 where the gap is 22 steps or more for sure
  P5 group maxima    M32 - delta of its tiles <= key2f(key) <= fp32_up(largest M32 + delta): the scans store the group
                     maximum UNROUNDED, as the ordered key of the fp32 value; groups that hold no tile have key 0
  P6 ragged end      an M-tile without real rows has code 15 and never decodes above bf16_up(M32 + delta); a 32-row tile
                     without real rows has mx = -inf; no word's maximum and no key is a NaN; no word is left at the sentinel
                     unless `may_skip` allows it

slack_g (P4), from the documented encoding alone.  The scan holds m in [M32 - delta, M32 + delta] and e in [M8_g - delta_g,
M8_g + delta_g] and encodes gs = (m - e) * 0.9999 / step.  Rounding down loses less than res steps (res = 1 for codes 0..7, 2
above), so steps * step >= 0.9999 (m - e) - res * step.  mx < m + ulp (one bf16 ulp of mx: the round-up).  Hence
  mx - steps step < m + ulp - 0.9999 (m - e) + res step = e + 1e-4 (m - e) + ulp + res step
                 <= M8_g + delta_g + 1e-4 gap_up + ulp_bf16(mx) + res step + f32          (gap_up = (M32 + delta) - (M8_g - delta_g))
with f32 = 2^-22 (|mx| + 32 step) for the fp32 roundings of encoder and decoder (m - e, the fma, 0.9999f / step, steps * step,
the final subtraction: each 2^-24 relative on a quantity below |mx| + 32 step).  A gap whose LOWER estimate
((M32 - delta) - (M8_g + delta_g)) * 0.9999 (1 - 2^-21) / step is 22 or more must come out as code 15; the inequality is not
asked there (the code saturates)."""
import numpy as np

U = 2.0 ** -24
GAMMA_384 = 384 * U / (1 - 384 * U)
F32_SLOP = 2.0 ** -22


# ------------------------------------------------------------------ number formats
def bf16_rne(x):
    """float32 array rounded to bf16 (nearest even), as float32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def f32_up(x):
    """smallest float32 >= x (x float64)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        y = x.astype(np.float32)
        low = y.astype(np.float64) < x
        return np.where(low, np.nextafter(y, np.float32(np.inf)), y).astype(np.float32)


def bf16_up_bits(m):
    """rr_scan_*: bf16 image of the float32 maximum, rounded toward +inf (+-inf stay)."""
    b = np.ascontiguousarray(m, dtype=np.float32).view(np.uint32)
    neg = (b >> np.uint32(31)) != 0
    return np.where(neg, b >> np.uint32(16), (b + np.uint32(0xFFFF)) >> np.uint32(16)).astype(np.uint32)


def bf16_val(bits):
    return (np.asarray(bits, dtype=np.uint32) << np.uint32(16)).view(np.float32)


def bf16_up(x):
    """smallest bf16 >= x (x float64), as float64."""
    return bf16_val(bf16_up_bits(f32_up(x))).astype(np.float64)


def key2f(k):
    """rr_key2f: the float32 an ordered key stands for."""
    k = np.asarray(k, dtype=np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return u.view(np.float32)


def f2key(f):
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


# ------------------------------------------------------------------ the encoding
def gap_step(eps):
    """rr_flt_gap_step: half the smallest finite positive error bound of the launch's queries (0: none), float32."""
    e = np.asarray(eps, dtype=np.float32)
    ok = (e > 0) & (e < np.float32(3.0e38))
    return np.float32(0.5) * e[ok].min() if ok.any() else np.float32(0.0)


def inv_step_of(step):
    return np.float32(0.9999) / np.float32(step) if step > 0 else np.float32(0.0)


def gap_code(m, e, inv_step):
    """rr_flt_gap_code: bits 20..23 of the float32 8 + (m - e) * inv_step, clamped to 31.99 (a NaN -- inf - inf -- gives 15)."""
    m = np.asarray(m, dtype=np.float32)
    e = np.asarray(e, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (m - e).astype(np.float32)
        g8 = (d.astype(np.float64) * np.float64(inv_step) + 8.0).astype(np.float32)      # (one fma)
        g8 = np.where(g8 == g8, np.minimum(g8, np.float32(31.99)), np.float32(31.99)).astype(np.float32)
    return (g8.view(np.uint32) >> np.uint32(20)) & np.uint32(15)


def gap_steps(code):
    """rr_flt_gap_steps: the decoder."""
    code = np.asarray(code).astype(np.int64)
    return np.where(code < 8, code, 2 * code - 8)


def encode_words(m8, eps):
    """The word of every (tile, query) from the scan's own float32 M-tile maxima m8[tile, 4, query]."""
    m8 = np.asarray(m8, dtype=np.float32)
    inv = inv_step_of(gap_step(eps))
    m32 = m8.max(axis=1)
    w = bf16_up_bits(m32)
    for g in range(4):
        w = w | (gap_code(m32, m8[:, g], inv) << np.uint32(16 + 4 * g))
    return w.astype(np.uint32)


def decode_words(words, step):
    """-> mx[tile, query] float32, codes[tile, 4, query], bound[tile, 4, query] float32 (rr_select_mtiles' arithmetic)."""
    w = np.asarray(words, dtype=np.uint32)
    mx = bf16_val(w & np.uint32(0xFFFF))
    codes = np.stack([(w >> np.uint32(16 + 4 * g)) & np.uint32(15) for g in range(4)], axis=1)
    with np.errstate(invalid="ignore"):
        bound = mx[:, None, :] - (gap_steps(codes).astype(np.float32) * np.float32(step)).astype(np.float32)
    return mx, codes, bound.astype(np.float32)


# ------------------------------------------------------------------ the float64 reference
def reference_m8(a_bf16, q_bf16, n_tiles32):
    """M8[tile, 4, query], delta[tile, 4, query] (float64) from bf16-valued rows [n, 384] and queries [nq, 384]."""
    a = np.asarray(a_bf16, dtype=np.float64)
    q = np.asarray(q_bf16, dtype=np.float64)
    n, nq = len(a), len(q)
    s = np.full((n_tiles32 * 32, nq), -np.inf)
    s[:n] = a @ q.T
    mag = np.zeros((n_tiles32 * 32, nq))
    mag[:n] = np.abs(a) @ np.abs(q).T
    return s.reshape(n_tiles32, 4, 8, nq).max(axis=2), GAMMA_384 * mag.reshape(n_tiles32, 4, 8, nq).max(axis=2)


def group_tiles(geom, gi):
    """32-row tiles [lo, hi) of selection group gi = wave * gpw + k (rr_scan_geom)."""
    gpw = max(int(geom["gpw"]), 1)
    wave, k = divmod(gi, gpw)
    t0 = wave * geom["tiles_per_wave"]
    t1 = min(t0 + geom["tiles_per_wave"], geom["n_tiles"])
    lo = t0 + k * geom["tiles_per_group"]
    hi = min(lo + geom["tiles_per_group"], t1)
    return (2 * lo, 2 * hi) if hi > lo else (0, 0)


def gap_upper_limit(m8, dl, low8, up32, mx, codes, step):
    """M8_g + slack_g of P4 (module docstring): the most a decoded bound may be, for M-tiles whose code is not saturated.
    m8, dl, low8 = m8 - dl, codes: [tile, 4, query]; up32 = (m8 + dl).max(axis=1), mx (float32): [tile, query]."""
    mx = np.ascontiguousarray(mx, dtype=np.float32)
    e_bits = (mx.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)
    ulp = np.ldexp(1.0, np.maximum(e_bits.astype(np.int64), 1) - 127 - 7)[:, None, :]          # one bf16 ulp of mx
    res = np.where(codes < 8, 1.0, 2.0)
    with np.errstate(invalid="ignore"):
        slack = dl + 1e-4 * (up32[:, None, :] - low8) + ulp + res * step + F32_SLOP * (np.abs(mx.astype(np.float64))[:, None, :] + 32 * step)
        return m8 + slack


# ------------------------------------------------------------------ the check
def check_words(words, keys, geom, M8, delta, eps, *, sentinel=None, may_skip=None, max_report=12, chunk=4096):
    """words[32-row tile, query] and keys[group, query] (or None) of ONE set against M8 / delta[tile, 4, query].
    -> (violations, stats).  A violation is a dict: prop, tile, query, sub (None for a whole word / a key: then `tile` is the
    group for P5), direction ('low' = the stored bound is BELOW what it must cover: unsafe; 'high' = looser than the
    encoding allows; 'nan', 'sentinel'), got, limit.  At most max_report per (prop, direction) are listed; stats["counts"] has
    them all, stats["tight_steps"] = worst (bound - M8) / step over the M-tiles P4's inequality is asked of,
    stats["safe_delta"] = worst (M8 - bound) / delta (P2 allows up to 1)."""
    words = np.asarray(words, dtype=np.uint32)
    T, nq = words.shape
    assert M8.shape == (T, 4, nq) and delta.shape == (T, 4, nq), (words.shape, M8.shape, delta.shape)
    step = np.float64(gap_step(eps))
    out, counts = [], {}
    stats = {"words": int(T * nq), "keys": 0, "sentinel_words": 0, "far": 0, "tight_steps": -np.inf, "safe_delta": -np.inf,
             "counts": counts, "step": float(step)}

    def report(prop, direction, mask, got, limit, t_off, has_sub):
        n_bad = int(mask.sum())
        if not n_bad:
            return
        counts[(prop, direction)] = counts.get((prop, direction), 0) + n_bad
        for idx in np.argwhere(mask):
            if sum(1 for v in out if v["prop"] == prop and v["direction"] == direction) >= max_report:
                break
            t, sub, q = (idx[0], idx[1], idx[2]) if has_sub else (idx[0], None, idx[1])
            out.append({"prop": prop, "tile": int(t + t_off), "query": int(q), "sub": None if sub is None else int(sub),
                        "direction": direction, "got": float(np.asarray(got)[tuple(idx)]), "limit": float(np.asarray(limit)[tuple(idx)])})

    lowM32_all = np.empty((T, nq))
    upM32_all = np.empty((T, nq))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t0 in range(0, T, chunk):
            sl = slice(t0, min(t0 + chunk, T))
            w, m8, dl = words[sl], M8[sl], delta[sl]
            empty = np.isneginf(m8)                                   # M-tiles without real rows
            low8, up8 = m8 - dl, m8 + dl
            low32, up32 = low8.max(axis=1), up8.max(axis=1)
            lowM32_all[sl], upM32_all[sl] = low32, up32
            skipped = np.zeros(w.shape, dtype=bool)
            if sentinel is not None:
                skipped = w == np.uint32(sentinel)
                stats["sentinel_words"] += int(skipped.sum())
                bad = skipped if may_skip is None else skipped & ~may_skip[sl]
                report("P6", "sentinel", bad, w, w, t0, False)
            mx, codes, bound = decode_words(w, step)
            mx64, bound64 = mx.astype(np.float64), bound.astype(np.float64)
            live = ~skipped
            report("P6", "nan", live & np.isnan(mx), mx, mx, t0, False)
            live &= ~np.isnan(mx)
            live3 = np.broadcast_to(live[:, None, :], m8.shape)
            # P1 / P3
            report("P1", "low", live & (mx64 < low32), mx64, low32, t0, False)
            lim3 = bf16_up(up32)
            report("P3", "high", live & (mx64 > lim3), mx64, lim3, t0, False)
            # P2
            real = live3 & ~empty
            report("P2", "low", real & (bound64 < low8), bound64, low8, t0, True)
            if real.any():
                r = np.where(real & (dl > 0), (m8 - bound64) / np.where(dl > 0, dl, 1.0), -np.inf)
                stats["safe_delta"] = max(stats["safe_delta"], float(r.max()))
            # P4
            if step > 0:
                far = ((low32[:, None, :] - up8) * 0.9999 * (1 - 2.0 ** -21) / step - 32 * 2.0 ** -23) >= 22.0
                report("P4", "high", real & far & (codes != 15), codes, np.full(codes.shape, 15), t0, True)
                stats["far"] += int((real & far).sum())
                lim4 = gap_upper_limit(m8, dl, low8, up32, mx, codes, step)
                near = real & ~far & np.isfinite(mx64)[:, None, :]
                report("P4", "high", near & (bound64 > lim4), bound64, lim4, t0, True)
                if near.any():
                    stats["tight_steps"] = max(stats["tight_steps"], float(np.where(near, (bound64 - m8) / step, -np.inf).max()))
            else:
                report("P4", "high", real & (codes != 0), codes, np.zeros(codes.shape), t0, True)
            # P6: M-tiles / tiles without real rows
            gone = live3 & empty
            report("P6", "high", gone & (codes != 15), codes, np.full(codes.shape, 15), t0, True)
            report("P6", "high", gone & (bound64 > lim3[:, None, :]), bound64, np.broadcast_to(lim3[:, None, :], m8.shape), t0, True)
            report("P6", "high", live & empty.all(axis=1) & ~np.isneginf(mx64), mx64, np.full(mx64.shape, -np.inf), t0, False)
        if keys is not None:
            keys = np.asarray(keys, dtype=np.uint32)
            ng = keys.shape[0]
            stats["keys"] = int(ng * nq)
            lo_g = np.full((ng, nq), -np.inf)
            up_g = np.full((ng, nq), -np.inf)
            has = np.zeros(ng, dtype=bool)
            for gi in range(ng):
                a, b = group_tiles(geom, gi)
                if b > a:
                    has[gi] = True
                    lo_g[gi], up_g[gi] = lowM32_all[a:b].max(axis=0), upM32_all[a:b].max(axis=0)
            hasq = np.broadcast_to(has[:, None], keys.shape)
            kv = key2f(keys).astype(np.float64)
            report("P5", "high", ~hasq & (keys != 0), keys, np.zeros(keys.shape), 0, False)
            isnan = hasq & (np.isnan(kv) | (keys > np.uint32(0xFF800000)) | (keys < np.uint32(0x007FFFFF)))
            report("P5", "nan", isnan, keys, keys, 0, False)
            ok = hasq & ~isnan
            report("P5", "low", ok & (kv < lo_g), kv, lo_g, 0, False)
            lim = f32_up(up_g).astype(np.float64)
            report("P5", "high", ok & (kv > lim), kv, lim, 0, False)
    return out, stats


def describe(violations, stats, limit=8):
    lines = [f"{n} x {p} ({d})" for (p, d), n in sorted(stats["counts"].items())]
    for v in violations[:limit]:
        where = f"tile {v['tile']}" if v["prop"] != "P5" else f"group {v['tile']}"
        sub = "" if v["sub"] is None else f" sub-tile {v['sub']}"
        lines.append(f"  {v['prop']} {v['direction']}: {where} query {v['query']}{sub}: got {v['got']!r}, limit {v['limit']!r}")
    return "\n".join(lines)
