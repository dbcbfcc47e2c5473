"""Texts for the review-cleaning kernel (csrc/rr_textprep.hip) and its model (textprep.model_clean), and the few lines of the
reference they are held against, restated: nlp/11_build_product_embeddings.py:22-39 (normalize_text, looks_spammy and their
three patterns) and :111-118 (the length filter, the spam filter, drop_duplicates)."""
import re

import numpy as np

MIN_TEXT_LEN, MAX_TEXT_LEN = 10, 4000                                                   # :22-23
URL_RE = re.compile(r"https?://\S+|www\.\S+", re.IGNORECASE)                            # :25
PROMO_RE = re.compile(r"(discount code|use code|sponsored|i received this.*free)", re.IGNORECASE)   # :26
REPEAT_RE = re.compile(r"(.)\1{9,}")                                                    # :27
PATTERN_LETTERS = sorted(set("httpswwwdiscountcodeusecodesponsoredireceivedthisfree"))


def ref_normalize(s: str) -> str:                                                       # :32-36
    s = s.replace("\r", " ").replace("\n", " ").strip()
    s = re.sub(r"\s+", " ", s)
    return s[:MAX_TEXT_LEN]


def ref_spammy(s: str) -> bool:                                                         # :38-39
    return (len(URL_RE.findall(s)) >= 2) or bool(PROMO_RE.search(s)) or bool(REPEAT_RE.search(s))


def ref_clean(s: str):
    """(normalised, short, spam) of one text."""
    t = ref_normalize(s)
    return t, len(t) < MIN_TEXT_LEN, ref_spammy(t)


def ref_keep(frame, no_spam=False, no_dedup=False):
    """:111-118 on a frame with sku and text: the index labels that survive, and the counts dropped as (short, spam, dup)."""
    df = frame[["sku", "text"]].copy()
    df["__txt"] = df["text"].map(ref_normalize)
    n0 = len(df)
    df = df[df["__txt"].str.len() >= MIN_TEXT_LEN]
    n1 = len(df)
    if not no_spam:
        df = df[~df["__txt"].apply(ref_spammy)]
    n2 = len(df)
    if not no_dedup:
        df = df.drop_duplicates(subset=["sku", "__txt"])
    return df.index.to_numpy(), (n0 - n1, n1 - n2, n2 - len(df))


FILL = "ab"                      # filler without whitespace, without a run and without a letter pair of the patterns' starts
E2, E3, E4 = "\u00e9", "\u4e2d", "\U0001F600"
PHRASES = ("discount code", "use code", "sponsored", "i received this", "free")
PREFIXES = ("http://", "https://", "www.")


def fill(n: int) -> str:
    return (FILL * (n // 2 + 1))[:n]


def crafted(window: int):
    """The list the issue asks for (more than 300 texts); `window` = the kernel's byte window."""
    t = ["", " ", " \t\r\n\u00a0\u2003\u3000 ", "a", " a ", "\n\nab\r\n"]
    # 9 and 10 code points of multi-byte characters, with and without whitespace around and inside
    for ch in (E2, E3, E4, "x"):
        alt = ch + ("y" if ch == "x" else "z")
        for k in (8, 9, 10, 11):
            body = (alt * k)[:k]
            t += [body, " " + body + "\u2003", body[:4] + " \n " + body[4:], body[:4] + "\u2028\u2029" + body[4:]]
    # the cut at 4000: inside a whitespace run, right behind a collapsed space, on a 4-byte character
    for head in range(3994, 4003):
        t += [fill(head) + "   \t " + fill(12), fill(head) + " " + fill(12), "  " + fill(head) + "\u3000\u3000" + E3 * 5,
              fill(head) + E4 + fill(3), fill(head) + E4 * 3, fill(head) + " " + E4 + " " + E4]
    # 4000 code points whose raw form is just under, at and just over the window (two 4-byte characters in turn)
    wide = (E4 + "\U0001F601") * 2000
    pad = window - len(wide.encode())
    for extra in (pad - 1, pad, pad + 1, pad + 40):
        t += [" " * extra + wide, wide + " " * extra, wide[:4000] + "\n" * (extra // 2) + "x" * (extra - extra // 2)]
    t += [fill(window - 5), fill(window), fill(window + 1), fill(3 * window)]
    # URLs
    urls = ["see http://a.b/c for more", "see http://a.b/c and https://d.e too", "http://", "ends with http://", "http:// www.",
            "www.", "this ends in www.", "http://ahttp://b", "wwww.x www.y", "wwww.x", "HTTP://A.B and WWW.C.D", "Https://x hTTp://y",
            "http://x", "http://x http://y", "www.a www.b", "www.a.www.b", "xhttp://a yhttps://b", "http:/x http:/y", "https:// x https:// y",
            "http://x\u00a0www.y", "http://x\u00a0 www.", "www..", "www. www. www.", "http://\u4e2d www.\u00e9", "hhttp://x wwww.y.",
            "a http://b", "www.x" + fill(30) + " " + fill(30) + "https://y", "http://http:// http://", "https://https://", "wWw.X Www.y"]
    t += [u + " " + fill(12) for u in urls] + [fill(12) + " " + u for u in urls]
    # promo phrases
    for p in PHRASES[:3]:
        mixed = "".join(c.upper() if i % 2 else c for i, c in enumerate(p))
        t += [p + " " + fill(10), mixed + " " + fill(10), fill(10) + p.upper(), fill(5) + " " + p[:-1] + " " + fill(9),
              p.replace(" ", "  ") + fill(10), p.replace(" ", "\u00a0") + fill(10), p.replace(" ", "\n") + fill(10), p[:3] + " " + p[3:] + fill(10)]
    recv = "i received this"
    t += [recv + " item for free", "free stuff: " + recv, recv + "free", "I Received This" + fill(20) + "FREE", recv + " fre e " + fill(5),
          "free " + recv + " free", recv + "\nproduct\tfor\u2003free", "ireceived this for free " + fill(4), recv[:-1] + " free " + fill(8),
          "i  received   this and it was free", recv + " fr" + fill(10), "fre" + recv + "e" + fill(10), recv + " " + recv + " fre", "free" + recv]
    # a phrase the cut splits, and one that just fits
    for p in PHRASES[:3] + (recv + " free",):
        for keep in (len(p) - 1, len(p), 3):
            t.append(fill(MAX_TEXT_LEN - keep - 1) + " " + p + " " + fill(6))
    t += [fill(3990) + " http://a www.b", fill(3984) + " http://a www.b", fill(3985) + " http://a www.", fill(3990) + "z" * 20,
          fill(3991) + "z" * 20, fill(3990) + " " + recv + " free", recv + " " + fill(3990) + " free"]
    # repeat runs
    for ch in ("z", "!", E2, E3, E4, "Z"):
        for k in (9, 10, 11, 25):
            t += [fill(6) + ch * k + fill(6), ch * k, "x" + ch * k, ch * k + "x"]
    t += ["aAaAaAaAaAaA bcd", "zzzzz zzzzz zzzzz", "zzzzz\u00a0\u00a0zzzzz", "..........", ". . . . . . . . . . .", E2 * 9 + "e\u0301" + fill(5),
          E3 * 5 + " " + E3 * 5, "\u4e2d\u4e2e" * 10, "\U0001F600\U0001F601" * 9]
    # the three code points IGNORECASE folds onto letters of the patterns
    t += ["\u0130 " + fill(12), "d\u0131scount code " + fill(5), "\u017fponsored " + fill(5), "u\u017fe code " + fill(5), fill(12) + "\u0130",
          "http\u017f://x http\u017f://y", "www.\u0131 www.\u0130"]
    return t


def random_texts(n: int, seed: int):
    """Texts over a small alphabet that makes hits likely: no code point the kernel leaves to the host, nothing near its
    window, so model_clean never answers needs_host for them."""
    units = ["discount", "use", "code", "sponsored", "i", "received", "this", "free", "http", "https", "://", "www", ".", "/", ":", "w",
             " ", " ", " ", " ", "\u00a0", "\u2003", "\n", E2, E3, E4, "a", "S", "E", "zzzzz", E3 * 5, "i received this", "discount code",
             "http://", "www."]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = int(rng.integers(1, 40))
        out.append("".join(units[i] for i in rng.integers(0, len(units), k)))
    return out


def boundary_variants(tile: int, per: int):
    """The constructs of crafted() laid across the kernel's tile edges and per-thread slice edges: every construct at every
    byte shift that makes it straddle the edge (and one before, one behind)."""
    constructs = [" \u2003\t\u00a0 ", E4, "z" * 10, E2 * 10, E3 * 10, E4 * 10, "z" * 9, "discount code", "use code", "sponsored",
                  "i received this free", "i received this x free", " http://x www.y ", " https://x https://y ", " WWW.x http://y ",
                  " http:// www. ", "x\u3000\u3000y", "\r\n"]
    edges = [per, 3 * per, tile - per, tile, tile + per, 2 * tile, 3 * tile]
    out = []
    for c in constructs:
        nb = len(c.encode())
        for e in edges:
            shifts = range(0, nb + 1) if e in (per, tile, 2 * tile) else (1, nb // 2, nb - 1)
            for d in shifts:
                if 0 <= d <= e:
                    out.append(fill(e - d) + c + fill(14) + " tail")
    return out
