"""The launch arithmetic of the token tail's non-GEMM kernels (csrc/tail.hip, reached through csrc/tail_api.hip), restated in
plain Python, and the shape classes it gives: LayerNorm, the set-Transformer attention `mha_small_*`, the three pooling families,
the survival head / loss kernels and the CAG middle.

This file holds the case tables of tests/test_gpu_tail_edges.py and shows on the CPU that they reach every class listed in
`WANTED` -- control flow that the suite's earlier case lists (written out literally below) never took -- that each row of a
table is needed for it, and the two facts about the dynamic LDS of `mha_small_*` that the launchers rely on.

`csrc/` is multimodal_path_omic_amd/csrc/; `:N` is a line of tail.hip, `api:N` one of tail_api.hip.
"""
import pytest

K_MAX_T = 16                 # :182 kMaxT
K_POOL_LONG_L = 64           # :183 kPoolLongL
K_MAX_C = 16                 # :597 kMaxC
K_MAX_BRANCHES = 4           # csrc/mpo_kernels.h:235 kMaxBranches
MHA_MAX_LDS = 160 * 1024     # :954 kMhaSmallMaxLds


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------- mha_small
def mha_lds(T, hd, backward):
    """:955-958 mha_small_lds = 4 waves x per_wave floats; per_wave :222 (forward) 3 T hd + 2 T^2 + 2 T, :293 (backward)
    4 T hd + 4 T^2"""
    per_wave = 4 * T * hd + 4 * T * T if backward else 3 * T * hd + 2 * T * T + 2 * T
    return 4 * per_wave * 4


def mha_forward_accepts(T, hd):
    """:960-967 mpo_check_mha_small, asked by the forward launcher (:972) and by mpo_encoder_forward before its first launch
    (api:193): the BACKWARD must fit (before: `lds <= 160 * 1024` on the forward's own size)"""
    return 1 <= T <= K_MAX_T and mha_lds(T, hd, True) <= MHA_MAX_LDS


def mha_backward_accepts(T, hd):
    """:984"""
    return 1 <= T <= K_MAX_T and mha_lds(T, hd, True) <= MHA_MAX_LDS


def mha(nb, ns, T, d, heads):
    """One launch of either kernel for B = nb * ns slides (api:221, api:286 pass BT)."""
    B, hd = nb * ns, d // heads
    wgs = cdiv(B * heads, 4)                                  # :974-975, :985-986 grid = (B H + 3) / 4, one wave per (slide, head)
    n = 3 * T * hd                                            # :192 values mha_load_head moves
    return dict(B=B, H=heads, hd=hd, T=T, wgs=wgs,
                live_last=B * heads - 4 * (wgs - 1),          # :226-227 gid = 4 blockIdx + wave, live = gid < B H
                n=n, rounds=cdiv(n, 12 * 64),                 # :193 768 values per round
                trips=cdiv(T * T, 64),                        # :233, :262, :307, :315 `it < T * T; it += 64`
                inst="<6, 32>" if T == 6 and hd == 32 else "<0, 0>",      # :974, :985
                lds_fwd=mha_lds(T, hd, False), lds_bwd=mha_lds(T, hd, True))


def mha_classes(nb, ns, T, d, heads):
    m = mha(nb, ns, T, d, heads)
    hd, got = m["hd"], set()
    if T == 1:
        got.add("mha T=1")
    if T * T == 64:
        got.add("mha T*T=64: one full score trip")
    if T * T > 64 and T * T % 64:
        got.add(f"mha {m['trips']} score trips, the last partial")
    if T == K_MAX_T:
        got.add("mha T=kMaxT")
    if hd & (hd - 1):
        got.add("mha head width not a power of two")            # :238, :319 rot = lane % hd
    if hd < 16:
        got.add("mha head width < 16")
    if hd > 64:
        got.add("mha head width > 64")
    if heads & (heads - 1):
        got.add("mha heads not a power of two")                  # :228, :301 gid / H, gid % H
    if heads == 1:
        got.add("mha one head")
    if m["live_last"] < 4:
        got.add(f"mha last workgroup: {m['live_last']} live wave(s) beside dead ones")
    if T != 6:
        got.add("mha <0, 0> at T != 6")
        if hd == 32:
            got.add("mha <0, 0> at head width 32")
        if m["n"] == 768:
            got.add("mha exactly one load round at T != 6")
        if 768 < m["n"] < 2 * 768:
            got.add("mha partial second load round at T != 6")
    if m["rounds"] >= 4 and m["n"] % 768 == 0:
        got.add("mha four or more full load rounds")
    if m["inst"] == "<6, 32>" and nb > 2:
        got.add(f"mha <6, 32> with {nb} branches")
    if m["lds_bwd"] > 64 * 1024:
        got.add("mha backward LDS > 64 KiB" + (", forward below" if m["lds_fwd"] <= 64 * 1024 else ""))
    if m["lds_fwd"] > 64 * 1024:
        got.add("mha forward LDS > 64 KiB")
    return got


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def ln(n_branches, rows_per_branch, d, aligned=True, with_params=True):
    """One backward launch (:921-941) over n_branches * rows_per_branch rows; the forward (:910-920) shares D4 and the row blocks."""
    rows = n_branches * rows_per_branch
    d4 = {256: 1, 512: 2}.get(d, 0) if aligned else 0         # :915-917, :936-938 `vec && d == 256 / 512`; vec: :905-909, :914, :935
    n_chunks = cdiv(rows_per_branch, 512) if with_params and rows_per_branch >= 2048 else 1      # :927
    per = cdiv(rows_per_branch, n_chunks)                     # :141
    cblocks = cdiv(d, 16)                                     # :175, :934
    return dict(D4=d4, n_chunks=n_chunks, per=per, cblocks=cblocks, last_cols=d - 16 * (cblocks - 1),     # :140, :144 col < d
                last_chunk_rows=rows_per_branch - per * (n_chunks - 1),      # :142 r1 = min(end of the branch, r0 + per)
                row_blocks=cdiv(rows, 4),                     # :171
                blocks=cdiv(rows, 4) + n_chunks * n_branches * cblocks)      # :934 (what = 3)


def ln_classes(nb, ns, T, d, aligned=True):
    R = ns * T
    g, got = ln(nb, R, d, aligned), set()
    chunked = g["n_chunks"] > 1
    if g["D4"] == 0 and d % 64:
        got.add("ln strided, d % 64 != 0")
    if g["D4"] == 0 and d < 64:
        got.add("ln strided, d < 64")
    if d % 16:
        got.add("ln ragged last column block, " + ("chunked" if chunked else "one chunk"))
    if g["D4"] == 0 and d == 256:
        got.add("ln strided at d = 256 (unaligned parameter)")
    if chunked and nb == 2:
        got.add("ln chunked, two branches")                   # :176 i % cblocks, (i / cblocks) % p.n, i / (cblocks p.n)
    if chunked and R == 2048:
        got.add("ln R = 2048 exactly: four chunks of 512" + (", two branches" if nb == 2 else ""))
    if chunked and g["last_chunk_rows"] < g["per"]:
        got.add("ln chunked, the last chunk short")
    if chunked and d != 256:
        got.add("ln chunked at a width other than 256")
    if 2048 - 64 <= R < 2048:
        got.add("ln one chunk just below 2048 rows")
    if nb == 3:
        got.add("ln three branches")
    if nb == K_MAX_BRANCHES:
        got.add("ln four branches: eight-member groups")      # api:147-154 launch_pairs, api:140 the limit
    return got


def encoder_classes(nb, ns, T, d, heads, ff, aligned=True):
    return (mha_classes(nb, ns, T, d, heads) if T <= K_MAX_T else set()) | ln_classes(nb, ns, T, d, aligned)


# ---------------------------------------------------------------------------------------------------------------- pooling
def pool_route(nb, L, d):
    """api:337 pool_fuses_scorer = n_branches <= 2 && L <= 64 && d <= 1024; otherwise :991, :1018 L > kPoolLongL"""
    if nb <= 2 and L <= 64 and d <= 1024:
        return "fused"
    return "long" if L > K_POOL_LONG_L else "short"


def wsum_trips(L):
    """:539-547 per row group rg = 0 .. 15: (unrolled trips `l + 112 < L; l += 128` from l = rg, tail trips `l < L; l += 16`)"""
    out = []
    for rg in range(16):
        l, unrolled, tail = rg, 0, 0
        while l + 7 * 16 < L:
            l, unrolled = l + 8 * 16, unrolled + 1
        while l < L:
            l, tail = l + 16, tail + 1
        out.append((unrolled, tail))
    return out


def trips_1024(L):
    """:510, :519, :527 (softmax), :583, :590 (d-scores): `l = tid; l < L; l += 1024` -> (trips, threads live in the last)"""
    trips = cdiv(L, 1024)
    return trips, L - 1024 * (trips - 1)


def pool_classes(nb, ns, L, d):
    route, got = pool_route(nb, L, d), set()
    if route == "fused":
        if L == 1:
            got.add("fused L=1")
        if 1 < L < 4:
            got.add("fused 1 < L < 4: idle waves")              # :433, :462 `l = wv; l < L; l += 4`
        if L == 4:
            got.add("fused L=4: one row per wave")
        if L == 63:
            got.add("fused L=63")
        if d % 64 and d % 4 == 0:
            got.add("fused d % 64 != 0")
        if d % 4:
            got.add("fused d % 4 != 0")
        if d == 64:
            got.add("fused d=64: 192 idle threads")             # :451 `c = tid; c < d; c += 256`
        if d == 1024:
            got.add("fused d=1024: the fuse boundary, four trips")
        elif d > 256:
            got.add(f"fused {cdiv(d, 256)} trips of the column loop")
    elif route == "short":
        if d > 1024:
            got.add("short d > 1024: " + ("L=1" if L == 1 else "L=64" if L == 64 else "1 < L < 64"))
        if nb > 2:
            got.add(f"short {nb} branches (forward only)")      # api:394 the backward refuses more than two
    else:
        trips = wsum_trips(L)
        some = sum(1 for u, _ in trips if u)
        if d % 16 and d >= 64:
            got.add("long d % 16 != 0")
        if d < 64:
            got.add("long d < 64")
        if 0 < some < 16:
            got.add("wsum: an unrolled trip for some row groups only")
        if L == 128:
            assert trips == [(1, 0)] * 16
            got.add("wsum: exactly one unrolled trip, no tail")
        if L == 129:
            assert trips == [(1, 1)] + [(1, 0)] * 15
            got.add("wsum: one unrolled trip and a one-row tail")
        if trips_1024(L) == (1, 1024):
            got.add("1024-thread kernels: exactly one trip")
        if trips_1024(L) == (2, 1):
            got.add("1024-thread kernels: a second trip of one row")
    return got


# ---------------------------------------------------------------------------------------------------------------- head, CAG
def head(B):
    """:1031 .. :1084 every head / loss launch: (B + 63) / 64 blocks of 64 threads, one thread per slide
    -> (blocks, threads live in the last one)"""
    blocks = cdiv(B, 64)
    return blocks, B - 64 * (blocks - 1)


def head_classes(B, C):
    got = {f"head C={C}"} if C in (1, 2, K_MAX_C) else set()
    blocks, live = head(B)
    if blocks == 2 and live < 64:
        got.add("head partial second block")
    if blocks >= 3:
        got.add("head three blocks")
    if B == 1:
        got.add("head one slide")
    return got


def cag_classes(hidden, rows):
    """:1118, :1125 one wave per row, (rows + 3) / 4 blocks, strided over `hidden`; the two LayerNorm parameter gradients
    go through :947-950 mpo_launch_ln_bwd_params_only (what = 2, w == nullptr) -> ln(1, rows, hidden)"""
    got = set()
    if hidden % 64:
        got.add("cag hidden % 64 != 0")
    if hidden == 64:
        got.add("cag hidden = 64: one strided trip")
    if rows == 1:
        got.add("cag one row")
    if rows % 4 == 1 and rows > 4:
        got.add("cag rows % 4 = 1 after a full block")
    if rows % 4 == 3:
        got.add("cag rows % 4 = 3")
    if ln(1, rows, hidden)["n_chunks"] > 1:
        got.add("cag rows >= 2048: chunked parameter gradient with w == nullptr")
    return got


# ---------------------------------------------------------------------------------------------------------------- the case tables
# (n_branches, n_slides, T, d, heads, ff); two layers
ENCODER_CASES = [
    (1, 1, 1, 256, 8, 512),        # T = 1
    (1, 3, 2, 96, 3, 64),          # B H = 9: three dead waves beside one live one; H = 3; hd = 32 at T != 6; d % 64 = 32; ff < 3 d
    (2, 1, 5, 64, 1, 128),         # one head; B H = 2; d = 64
    (1, 5, 7, 100, 4, 100),        # hd = 25; d % 16 = 4 and d % 64 != 0
    (1, 2, 3, 16, 8, 32),          # hd = 2; d < 64
    (2, 2, 8, 256, 8, 512),        # T T = 64; 768 loaded values, exactly one round
    (2, 3, 9, 256, 8, 512),        # T T = 81; 864 values: a partial second round
    (2, 1, 16, 256, 8, 512),       # T = kMaxT
    (1, 2, 16, 512, 8, 512),       # hd = 64 at T = 16: four load rounds; D4 = 2
    (1, 1, 16, 128, 1, 256),       # hd = 128: dynamic LDS 107 008 B forward, 147 456 B backward
    (3, 2, 6, 256, 8, 512),        # three branches on <6, 32>
    (4, 2, 6, 256, 8, 512),        # four branches: eight-member groups
    (2, 128, 16, 256, 8, 512),     # R = 2048: four chunks of 512, two branches
    (2, 170, 12, 256, 8, 512),     # R = 2040: one chunk of 2040 rows
    (2, 187, 11, 256, 8, 512),     # R = 2057: five chunks, the last one short; T T = 121; 1056 loaded values
    (1, 128, 16, 100, 4, 100),     # chunks on the strided LayerNorm, with a ragged column block
]
LDS_CASE = (1, 1, 16, 128, 1, 256)                  # the one launch with a forward above 64 KiB
UNALIGNED_CASE = (2, 5, 6, 256, 8, 512)             # norm1.weight of one branch one float into its storage: D4 = 0 at d = 256
UNALIGNED_PARAM = (1, "enc.layers.0.norm1.weight")  # (branch, state_dict name)
FIVE_BRANCHES = (5, 1, 6, 256, 8, 512)              # refused before any launch (api:186)
LDS_REFUSED = (1, 1, 16, 160, 1, 256)               # forward fits (131 584 B), backward does not (180 224 B): refused in the forward
# rows whose classes other rows reach as well, and why they stay
ENCODER_SHARED = {
    (2, 3, 9, 256, 8, 512): "the smallest T T > 64 (54 rows); (2, 187, 11, ...) reaches its classes only at 4114 rows",
    (2, 1, 16, 256, 8, 512): "T = kMaxT alone: every other T = 16 row adds a head width, an LDS size or row chunks to it",
}

# (n_branches, n_slides, L, d) -> modes: "both" (eval and training), "eval"; layouts: plain, and interleaved where d % 4 == 0
POOL_FUSED = [(2, 1, 1, 256), (2, 3, 3, 256), (1, 2, 4, 256), (2, 1, 5, 100), (2, 1, 6, 64), (2, 5, 6, 512), (2, 2, 63, 256),
              (1, 1, 64, 1024)]
POOL_FUSED_EVAL_PLAIN = [(1, 2, 6, 102)]
POOL_SHORT = [(1, 2, 6, 1028), (2, 1, 64, 1028), (1, 1, 1, 1028)]
POOL_SHORT_FORWARD_ONLY = [(3, 2, 6, 256), (4, 1, 6, 256)]
POOL_LONG = [(2, 1, 65, 100), (1, 2, 113, 256), (2, 1, 128, 256), (1, 1, 129, 256), (1, 2, 1024, 256), (2, 1, 1025, 256),
             (1, 1, 130, 40)]
POOL_CASES = POOL_FUSED + POOL_FUSED_EVAL_PLAIN + POOL_SHORT + POOL_SHORT_FORWARD_ONLY + POOL_LONG
POOL_REFUSED_INTERLEAVED = (1, 2, 6, 102)           # api:343 interleaved h needs d % 4 == 0

HEAD_C = (1, 2, 16)
HEAD_B = (1, 65, 130)
HEAD_C_REFUSED = 17

# (hidden, rows); dim = hidden: every pair of the small grid, and three single cases
CAG_GRID_HIDDEN = (64, 100)
CAG_GRID_ROWS = (1, 5)
CAG_OTHER = [(256, 130), (256, 2052), (512, 7)]


def cag_table(hidden=CAG_GRID_HIDDEN, rows=CAG_GRID_ROWS, other=None):
    return [(h, r) for h in hidden for r in rows] + list(CAG_OTHER if other is None else other)


def head_table(cs=HEAD_C, bs=HEAD_B):
    return [(b, c) for c in cs for b in bs]


CAG_CASES = cag_table()
# what stays although the rest of its table reaches its classes, and why
HEAD_SHARED = {("B", 1): "one slide, the smallest launch: the earlier lists have it at C = 4 only"}
CAG_SHARED = {(256, 130): "the model's width between one block and the chunk threshold, at a row count that is no multiple of 6"}

WANTED = {
    "encoder": {
        "mha T=1", "mha T*T=64: one full score trip", "mha 2 score trips, the last partial", "mha 3 score trips, the last partial",
        "mha T=kMaxT", "mha head width not a power of two", "mha head width < 16", "mha head width > 64",
        "mha heads not a power of two", "mha one head", "mha last workgroup: 1 live wave(s) beside dead ones",
        "mha last workgroup: 2 live wave(s) beside dead ones", "mha <0, 0> at T != 6", "mha <0, 0> at head width 32",
        "mha exactly one load round at T != 6", "mha partial second load round at T != 6", "mha four or more full load rounds",
        "mha <6, 32> with 3 branches", "mha <6, 32> with 4 branches", "mha backward LDS > 64 KiB, forward below", "mha backward LDS > 64 KiB",
        "mha forward LDS > 64 KiB",
        "ln strided, d % 64 != 0", "ln strided, d < 64", "ln ragged last column block, one chunk",
        "ln ragged last column block, chunked", "ln strided at d = 256 (unaligned parameter)", "ln chunked, two branches",
        "ln R = 2048 exactly: four chunks of 512", "ln R = 2048 exactly: four chunks of 512, two branches",
        "ln chunked, the last chunk short", "ln chunked at a width other than 256",
        "ln one chunk just below 2048 rows", "ln three branches", "ln four branches: eight-member groups"},
    "pool": {
        "fused L=1", "fused 1 < L < 4: idle waves", "fused L=4: one row per wave", "fused L=63", "fused d % 64 != 0",
        "fused d % 4 != 0", "fused d=64: 192 idle threads", "fused d=1024: the fuse boundary, four trips",
        "fused 2 trips of the column loop", "short d > 1024: L=1", "short d > 1024: L=64", "short d > 1024: 1 < L < 64",
        "short 3 branches (forward only)", "short 4 branches (forward only)", "long d % 16 != 0", "long d < 64",
        "wsum: an unrolled trip for some row groups only", "wsum: exactly one unrolled trip, no tail",
        "wsum: one unrolled trip and a one-row tail", "1024-thread kernels: exactly one trip",
        "1024-thread kernels: a second trip of one row"},
    "head": {"head C=1", "head C=2", "head C=16", "head partial second block", "head three blocks"},
    "cag": {"cag hidden % 64 != 0", "cag hidden = 64: one strided trip", "cag one row", "cag rows % 4 = 1 after a full block",
            "cag rows % 4 = 3", "cag rows >= 2048: chunked parameter gradient with w == nullptr"},
}


def encoder_table():
    """(case, aligned) of every encoder run of the GPU file"""
    return [(c, True) for c in ENCODER_CASES] + [(UNALIGNED_CASE, False)]


def reached(family, table):
    got = set()
    for row in table:
        if family == "encoder":
            case, aligned = row
            got |= encoder_classes(*case, aligned=aligned)
        else:
            got |= {"pool": pool_classes, "head": head_classes, "cag": cag_classes}[family](*row)
    return got


TABLES = {"encoder": encoder_table(), "pool": POOL_CASES, "head": head_table(), "cag": CAG_CASES}
SHARED = {"encoder": {(c, True): why for c, why in ENCODER_SHARED.items()}, "pool": {}, "head": HEAD_SHARED, "cag": CAG_SHARED}


def deletions(family):
    """(what is deleted, the table without it): every row of a list, every value of an axis of a grid"""
    if family == "head":
        return ([(("C", c), head_table(cs=[v for v in HEAD_C if v != c])) for c in HEAD_C]
                + [(("B", b), head_table(bs=[v for v in HEAD_B if v != b])) for b in HEAD_B])
    if family == "cag":
        return ([(("hidden", h), cag_table(hidden=[v for v in CAG_GRID_HIDDEN if v != h])) for h in CAG_GRID_HIDDEN]
                + [(("rows", r), cag_table(rows=[v for v in CAG_GRID_ROWS if v != r])) for r in CAG_GRID_ROWS]
                + [(row, cag_table(other=[v for v in CAG_OTHER if v != row])) for row in CAG_OTHER])
    table = TABLES[family]
    return [(row, table[:i] + table[i + 1:]) for i, row in enumerate(table)]


# ---------------------------------------------------------------------------------------------------------------- the tests
def test_restated_arithmetic_on_known_shapes():
    # the model's own shape: 2 branches x 32 slides x 6 tokens, d = 256, 8 heads
    m = mha(2, 32, 6, 256, 8)
    assert (m["inst"], m["wgs"], m["live_last"], m["n"], m["rounds"], m["trips"]) == ("<6, 32>", 128, 4, 576, 1, 1)
    assert (m["lds_fwd"], m["lds_bwd"]) == (4 * (576 + 72 + 12) * 4, 4 * (768 + 144) * 4)
    assert ln(2, 192, 256) == dict(D4=1, n_chunks=1, per=192, cblocks=16, last_cols=16, last_chunk_rows=192, row_blocks=96,
                                   blocks=96 + 32)
    # the issue's figures
    m = mha(*LDS_CASE[:5])
    assert (m["lds_fwd"], m["lds_bwd"], m["rounds"], m["live_last"]) == (107008, 147456, 8, 1)
    assert [mha(*c[:5])["n"] for c in ENCODER_CASES[5:7]] == [768, 864] and mha(2, 187, 11, 256, 8)["n"] == 1056
    assert mha(1, 3, 2, 96, 3)["wgs"] == 3 and mha(1, 3, 2, 96, 3)["live_last"] == 1          # B H = 9
    assert mha(1, 2, 16, 512, 8)["rounds"] == 4 and mha(1, 2, 16, 512, 8)["lds_bwd"] == 81920
    g = ln(2, 2057, 256)
    assert (g["n_chunks"], g["per"], g["last_chunk_rows"]) == (5, 412, 409)
    assert ln(2, 2048, 256)["n_chunks"] == 4 and ln(2, 2048, 256)["per"] == 512 and ln(2, 2040, 256)["n_chunks"] == 1
    assert ln(1, 2050, 256)["per"] * 5 == 2050                                                   # the old chunked case: five equal chunks
    g = ln(1, 2048, 100)
    assert (g["D4"], g["cblocks"], g["last_cols"], g["n_chunks"]) == (0, 7, 4, 4)
    assert ln(1, 2052, 256, with_params=True)["n_chunks"] == 5                                   # CAG at 2052 rows
    assert [pool_route(*c) for c in ((2, 64, 1024), (2, 64, 1028), (3, 6, 256), (2, 65, 256), (4, 65, 256))] == \
        ["fused", "short", "short", "long", "long"]
    assert wsum_trips(112) == [(0, 7)] * 16 and wsum_trips(65) == [(0, 5)] + [(0, 4)] * 15
    assert wsum_trips(113) == [(1, 0)] + [(0, 7)] * 15 and wsum_trips(127) == [(1, 0)] * 15 + [(0, 7)]
    assert wsum_trips(130) == [(1, 1)] * 2 + [(1, 0)] * 14
    # every row of a bag is summed exactly once, whatever the cut
    for L in (65, 112, 113, 127, 128, 129, 130, 333, 1024, 1025, 2050, 3000):
        assert sum(8 * u + t for u, t in wsum_trips(L)) == L, L
    assert [trips_1024(L) for L in (65, 1024, 1025, 2050, 3000)] == [(1, 65), (1, 1024), (2, 1), (3, 2), (3, 952)]
    assert [head(b) for b in (1, 64, 65, 130)] == [(1, 1), (1, 64), (2, 1), (3, 2)]


def test_backward_lds_is_never_below_the_forward():
    """per wave the backward needs T (hd + 2 T - 2) floats more: a geometry whose backward fits has a forward that fits"""
    for T in range(1, K_MAX_T + 1):
        for hd in range(1, 1025):
            assert mha_lds(T, hd, True) - mha_lds(T, hd, False) == 16 * T * (hd + 2 * T - 2) >= 0, (T, hd)


def test_lds_window_the_two_launchers_used_to_treat_differently():
    """Before the forward asked for the backward's size: at T = 16 head widths 145 .. 202 passed `lds <= 160 KiB` in the forward
    and failed it in the backward -- d = 160 with one head ran a training step's forward and died in its backward."""
    old_forward = [hd for hd in range(1, 1025) if mha_lds(16, hd, False) <= MHA_MAX_LDS]
    backward = [hd for hd in range(1, 1025) if mha_backward_accepts(16, hd)]
    assert [hd for hd in old_forward if hd not in backward] == list(range(145, 203))
    assert backward == list(range(1, 145))
    for T in range(1, K_MAX_T + 1):
        for hd in range(1, 1025):
            assert mha_forward_accepts(T, hd) == mha_backward_accepts(T, hd)
    nb, ns, T, d, heads, _ = LDS_REFUSED
    assert mha_lds(T, d // heads, False) == 131584 <= MHA_MAX_LDS < mha_lds(T, d // heads, True) == 180224
    assert not mha_forward_accepts(T, d // heads) and mha_forward_accepts(*[LDS_CASE[2], LDS_CASE[3] // LDS_CASE[4]])


@pytest.mark.parametrize("family", list(TABLES))
def test_case_table_reaches_every_class(family):
    got = reached(family, TABLES[family])
    print(f"{family}: {sorted(got)}")
    assert got >= WANTED[family], sorted(WANTED[family] - got)


@pytest.mark.parametrize("family", list(TABLES))
def test_every_row_of_a_table_is_needed(family):
    """Without any one row (or value of a grid's axis) some wanted class is reported missing -- except what is listed as shared,
    which must exist."""
    what = [w for w, _ in deletions(family)]
    assert set(SHARED[family]) <= set(what)
    for w, table in deletions(family):
        missing = WANTED[family] - reached(family, table)
        if w in SHARED[family]:
            assert not missing, (w, missing)
        else:
            assert missing, f"{family}: {w} carries no class of its own"


def test_a_case_removed_from_a_table_is_noticed():
    """The coverage check is not vacuous: what is reported without a given row."""
    def without(family, drop):
        return WANTED[family] - reached(family, [r for r in TABLES[family] if not drop(r)])
    assert without("encoder", lambda r: False) == set()
    assert without("encoder", lambda r: r[0] == (1, 1, 1, 256, 8, 512)) == {"mha T=1"}
    # (one live wave beside three dead ones: the hd = 128 row has that too, on its only workgroup)
    assert without("encoder", lambda r: r[0] == (1, 3, 2, 96, 3, 64)) == {"mha heads not a power of two"}
    assert without("encoder", lambda r: r[0][2] in (9, 11)) == {"mha 2 score trips, the last partial",
                                                                "ln chunked, the last chunk short"}
    assert without("encoder", lambda r: not r[1]) == {"ln strided at d = 256 (unaligned parameter)"}
    assert without("encoder", lambda r: r[0] == LDS_CASE) == {"mha forward LDS > 64 KiB", "mha backward LDS > 64 KiB",
                                                               "mha head width > 64"}
    assert without("pool", lambda r: r[2] == 129) == {"wsum: one unrolled trip and a one-row tail"}
    assert without("pool", lambda r: r[3] == 1028) == {"short d > 1024: L=1", "short d > 1024: L=64", "short d > 1024: 1 < L < 64"}
    assert without("pool", lambda r: r[0] > 2) == {"short 3 branches (forward only)", "short 4 branches (forward only)"}
    assert WANTED["head"] - reached("head", head_table(bs=(1, 65))) == {"head three blocks"}
    assert WANTED["head"] - reached("head", head_table(cs=(1, 2))) == {"head C=16"}
    assert without("cag", lambda r: r[1] == 2052) == {"cag rows >= 2048: chunked parameter gradient with w == nullptr"}
    assert without("cag", lambda r: r[0] == 100) == {"cag hidden % 64 != 0"}


def test_what_the_earlier_case_lists_reached():
    """The gap.  The case lists of tests/test_gpu_train_dropout.py, tests/test_gpu_tail.py, tests/test_gpu_sct_loss.py and
    tests/golden/cases.py, written out: none of them reaches a single wanted class.  (One model-level test does reach a few:
    see `model_level` below.)"""
    old_encoder = ([(2, ns, 6, d, 8, 512) for ns in (1, 5, 32) for d in (128, 256, 512)]          # token tail, fast and general
                   + [(2, 1, 17, 256, 8, 512), (2, 1, 200, 256, 8, 512), (1, 1, 2050, 256, 8, 512)]    # bag rows (T > 16)
                   + [(2, 5, 6, 128, 8, 100), (2, 5, 6, 128, 8, 102)]                              # irregular ff
                   + [(2, 5, 6, 256, 8, 512), (1, 1, 200, 256, 8, 512)]                            # epoch; controls
                   + [(1, 1, 6, 256, 8, 512), (1, 3, 6, 256, 8, 512), (2, 32, 6, 256, 8, 512)]      # test_gpu_tail.py
                   + [(1, 1, 333, 256, 8, 512), (1, 1, 3000, 256, 8, 512)])                        # cases.GE_MODEL_CASES
    got = reached("encoder", [(c, True) for c in old_encoder])
    assert not got & WANTED["encoder"], sorted(got & WANTED["encoder"])
    small = [c for c in old_encoder if c[2] <= K_MAX_T]
    assert {(c[2], c[4]) for c in small} == {(6, 8)}                                               # T = 6 and 8 heads, always
    assert {mha(*c[:5])["inst"] for c in small if c[3] == 256} == {"<6, 32>"}
    assert {c[3] // c[4] for c in small if mha(*c[:5])["inst"] == "<0, 0>"} == {16, 64}
    assert all(mha(*c[:5])["live_last"] == 4 for c in small)                                       # B H % 4 == 0
    assert {c[3] for c in old_encoder if ln(c[0], c[1] * c[2], c[3])["D4"] == 0} == {128}
    assert [(c[0], c[1] * c[2], c[3]) for c in old_encoder if ln(c[0], c[1] * c[2], c[3])["n_chunks"] > 1] == \
        [(1, 2050, 256), (1, 3000, 256)]
    assert max(c[0] for c in old_encoder) == 2

    # Not blind everywhere: tests/test_gpu_models.py::test_other_omic_group_counts_and_tiny_bags sends 2 branches x 6 slides of
    # T = 1, 3, 7, 8, 9, 15, 16 tokens through a whole model -- eval mode, d = 256 and eight heads only, behind the model's bars
    model_level = [(2, 6, T, 256, 8, 512) for T in (1, 3, 7, 8, 9, 15, 16)]
    assert reached("encoder", [(c, True) for c in model_level]) & WANTED["encoder"] == {
        "mha T=1", "mha T*T=64: one full score trip", "mha 2 score trips, the last partial", "mha T=kMaxT", "mha <0, 0> at T != 6",
        "mha <0, 0> at head width 32", "mha exactly one load round at T != 6", "mha partial second load round at T != 6"}
    assert reached("pool", [c[:3] + (256,) for c in model_level]) & WANTED["pool"] == {"fused L=1", "fused 1 < L < 4: idle waves"}

    old_pool = ([(2, ns, L, 256) for L in (6, 64, 65) for ns in (1, 32)] + [(2, 1, 2050, 256)]     # training, both layouts
                + [(2, 32, 6, 256), (2, 32, 64, 256), (1, 1, 65, 256)]                             # rho zeros, controls, epoch
                + [(1, 1, 6, 256), (1, 1, 3000, 256), (1, 3, 6, 256), (2, 5, 6, 256)]              # test_gpu_tail.py, cases.POOL_CASES
                + [(1, 1, 333, 256), (1, 1, 2050, 256)])                                           # gene-expression model
    got = reached("pool", old_pool)
    assert not got & WANTED["pool"], sorted(got & WANTED["pool"])
    assert "short" not in {pool_route(c[0], c[2], c[3]) for c in old_pool}                         # pool_fwd / pool_bwd_kernel: never
    assert {c[2] for c in old_pool if pool_route(c[0], c[2], c[3]) == "fused"} == {6, 64}
    assert {c[2] for c in old_pool if pool_route(c[0], c[2], c[3]) == "long"} == {65, 333, 2050, 3000}
    assert all(u == 0 for u, _ in wsum_trips(65))                                                  # of the wsum classes only L <= 112

    old_head = [(b, 4) for b in (1, 3, 8, 17, 64, 5, 16, 32, 4)]
    got = reached("head", old_head)
    assert not got & WANTED["head"], sorted(got & WANTED["head"])
    assert all(head(b)[0] == 1 for b, _ in old_head)

    old_cag = [(h, 6 * n) for h in (128, 256, 512) for n in (1, 4, 32)]
    got = reached("cag", old_cag)
    assert not got & WANTED["cag"], sorted(got & WANTED["cag"])
