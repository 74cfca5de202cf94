"""Shared by test_batch_shapes_cpu.py, test_gpu_batch_shapes.py and test_gpu_encoder_batch_shapes.py: what a BATCH changes in the plan of k_gemm_nt (uniform
batches of the encoder, ragged groups of the post-net) on top of gemm_shapes.plan, the plan of the cooperative encoder BiLSTM
as a function of the batch and the device's CU count, the cases that reach every class of either, pools of distinct chunks,
and the references (fp64 oracle per chunk, and the fp32 oracle's own distance from it), computed once.

The rules restated here (the GEMM's own are in gemm_shapes.plan, which takes a list of per-item row counts):

  k_gemm_nt, batch   split-K: grid z = item x K slice, the workspace and the tickets indexed by (item, row tile, column tile);
                     XCD mapping: the row tiles of all items numbered through, eight consecutive ones to a group, the last
                     group padded with blocks that exit; a ragged item with fewer row tiles than the longest exits early
                     under the plain mapping; the last post-net layer stores transposed, into one (80 x sum F) matrix at a
                     column offset per item or into one dense (80 x F) matrix per item.
  run_postnet        at most GEMM_RAGGED_MAX = 64 items per launch; postnet_groups walks a larger batch group by group.
  launch_bilstm_coop G = CUs / 8 groups of eight workgroups per launch (tacotron2_handle.cpp: coop_group).  B <= G: one chunk
                     per group.  B > G: two chunks per group (k_bilstm_coop<2>), the last group of an odd launch holds one;
                     2 G chunks per launch, so B > 2 G takes several launches with b0 = 2 G, 4 G, ... over one exchange
                     buffer zeroed again in between.  The hidden state crosses T - 1 times, in two slots by step parity.
"""
import time

import numpy as np

import gemm_shapes as gs

GEMM_RAGGED_MAX = gs.GEMM_RAGGED_MAX  # csrc/kernels.h
CU_PER_GROUP = 8                      # csrc/tacotron2_handle.cpp: coop_group = cus / 8
G_MI355X = 32                         # 256 CUs
SEED = 20240327
ENC_SITES = gs.ENTRIES["encoder"][0]
POST_SITES = gs.ENTRIES["postnet"][0]


# ---- the GEMM's batch classes ------------------------------------------------------------------------------------------

def gemm_classes(site, Mz):
    """The classes a launch of the items Mz (row counts, two or more) takes at `site`: the plan (tile, mapping, slices, fill of
    the last group of 8) and what only a batch can reach."""
    Mz = list(Mz)
    assert len(Mz) >= 2
    p = gs.plan(site, Mz)
    tile = p["tile"]
    base = "%s:t%d:%s:s%d" % (site, tile, p["mapping"], p["slices"])
    c = set()
    if p["mapping"] == "xcd":
        base += ":groups-%s" % ("padded" if p["padded"] else "of-8")
        if min(Mz) < tile:
            c.add(base + "+short-item")            # an item of less than one tile among the tiles numbered through
        ends = np.cumsum([gs.cdiv(m, tile) for m in Mz])[:-1]
        if np.any(ends % 8 != 0):
            c.add(base + "+boundary-in-group")     # a group of 8 row tiles holds tiles of two items
    if p["slices"] > 1:
        c.add(base + "+items")                     # blockIdx.z = item x slice, tickets and workspace across items
        if min(gs.cdiv(m, tile) for m in Mz) < gs.cdiv(max(Mz), tile):
            c.add(base + "+early-return")          # grid rows past a short item's end exit before they take a ticket
    elif p["mapping"] == "plain" and min(gs.cdiv(m, tile) for m in Mz) < gs.cdiv(max(Mz), tile):
        c.add(base + "+early-return")
    c.add(base)
    return c


def encoder_classes(B, T):
    return set().union(*(gemm_classes(s, [T] * B) for s in ENC_SITES))


def groups_of(Fs):
    Fs = list(Fs)
    return [Fs[b:b + GEMM_RAGGED_MAX] for b in range(0, len(Fs), GEMM_RAGGED_MAX)]


def postnet_classes(Fs):
    """Every group's classes at the three sites, the number of groups, and both stores of the last layer (a case runs both)."""
    gr = groups_of(Fs)
    c = {"groups:%d" % len(gr), "post4:store-offset", "post4:store-dense"}
    for g in gr:
        if len(g) >= 2:
            for s in POST_SITES:
                c |= gemm_classes(s, g)
    return c


# ---- the cooperative BiLSTM's plan ---------------------------------------------------------------------------------------

def coop_group(cus):
    return max(cus // CU_PER_GROUP, 1)


def bilstm_plan(B, G):
    """run_encoder + launch_bilstm_coop for B chunks on a device of G groups."""
    slots = (B + 1) // 2 if B > G else B
    launches = gs.cdiv(slots, G)
    group = G if B > G else gs.cdiv(B, launches)
    nc = 2 if B > group else 1
    per_launch = nc * group
    b0 = tuple(range(0, B, per_launch))
    n = tuple(min(per_launch, B - b) for b in b0)
    return dict(NC=nc, launches=len(b0), b0=b0, chunks=n, groups=tuple(gs.cdiv(x, nc) for x in n),
                exchange_chunks=2 * group, last_group_single=bool(nc == 2 and n[-1] % 2 == 1))


def bilstm_class(B, G):
    p = bilstm_plan(B, G)
    c = "nc%d:launches-%d" % (p["NC"], p["launches"])
    if p["NC"] == 1:
        return c + (":all-groups" if B == G else "")
    c += ":last-group-%s" % ("single" if p["last_group_single"] else "pair")
    return c + (":all-groups" if p["launches"] == 1 and B == 2 * G else "")


def exchange_class(T):
    return {1: "no-exchange", 2: "one-exchange"}.get(T, "both-slots")


BILSTM_B = ("2", "G", "G+1", "2G-1", "52", "2G", "2G+1", "2G+2")


def bilstm_batches(G):
    """name -> (B, the class it is there for) of the BiLSTM sweep on a device of G groups (52: the batch of BASELINE configs[3],
    two chunks per group in one launch where G < 52 < 2 G; elsewhere whatever plan it takes)."""
    return {"2": (2, "nc1:launches-1" + (":all-groups" if G == 2 else "")), "G": (G, "nc1:launches-1:all-groups"),
            "G+1": (G + 1, "nc2:launches-1:last-group-single"), "2G-1": (2 * G - 1, "nc2:launches-1:last-group-single"),
            "52": (52, "nc2:launches-1:last-group-pair" if G < 52 < 2 * G else bilstm_class(52, G)),
            "2G": (2 * G, "nc2:launches-1:last-group-pair:all-groups"), "2G+1": (2 * G + 1, "nc2:launches-2:last-group-single"),
            "2G+2": (2 * G + 2, "nc2:launches-2:last-group-pair")}


BILSTM_T = (1, 2, 3, 5, 17)

# ---- the sweeps ----------------------------------------------------------------------------------------------------------
# encoder (B, T): what each is there for (test_batch_shapes_cpu.py checks the classes)
ENCODER_CASES = (
    (2, 1), (9, 1), (11, 1), (17, 1), (65, 1),   # enc_conv at s4 / s3 / s2 / s1 and on 64x64 tiles, plain; memory at s2 / s1, plain
    (33, 1),                                     # bilstm_proj on 64x64 tiles, plain
    (2, 65), (4, 33),                            # memory XCD-mapped, groups padded and of 8
    (61, 17), (16, 65),                          # bilstm_proj on 64x64 tiles, XCD-mapped, groups padded and of 8
    (22, 48), (24, 48),                          # bilstm_proj on 32x32 tiles, XCD-mapped
    (41, 63), (26, 100),                         # enc_conv on 32x32 tiles, XCD-mapped
    (40, 65), (41, 65),                          # enc_conv on 64x64 tiles, XCD-mapped
    # chunks of less than one tile under the XCD mapping: 64x64 tiles with the groups of 8 and padded (enc_conv, bilstm_proj), 32x32 (memory)
    (64, 41), (65, 41), (8, 17),
)
ENC_B_MAX, ENC_T_MAX = 66, 128  # the space the coverage test enumerates


def _cycle(values, n):
    return tuple(values[i % len(values)] for i in range(n))


_MANY = (33,) + _cycle((3, 1, 2, 7, 5, 12, 4, 9), 129)  # 64 of them: 65 row tiles of 32 in 368 frames
_TINY = _cycle((1, 2, 3), 63)
POSTNET_CASES = {
    "pair": (40, 17),
    "five": (12, 30, 7, 22, 16),
    "five-longest-first": (30, 22, 16, 12, 7),
    "tiles10-s3": (100, 40, 33, 12, 7),
    "tiles12-s2": (40,) * 6,
    "tiles13-s2": (100, 100, 40, 12, 7, 5),
    "tiles17-s1": (33,) * 8 + (1,),
    "sum400": (100, 100, 100, 100),
    "sum401": (101, 100, 100, 100),
    "sum438-short": (1, 193, 101, 100, 3, 2, 1, 7, 5, 12, 4, 9),
    "n51-post4-s3": (40,) + _MANY[1:51],
    "n50-sum2560": (64,) * 23 + (41,) * 8 + (40,) * 19,
    "n50-sum2561": (64,) * 23 + (41,) * 9 + (40,) * 18,
    "n52-sum2613": (64,) * 23 + (41,) * 9 + (40,) * 19 + (12,),
    "n53-sum2620": (64,) * 23 + (41,) * 9 + (40,) * 19 + (12, 7),
    "n64-sum2560": (40,) * 64,
    "n64-sum2561": (41,) + (40,) * 63,
    "n64-sum2620": (40,) * 63 + (100,),
    "n64-one-long": (193,) + _TINY,
    "n64-two-long-sum417": (193, 100) + _TINY[:62],
    "n64-one-long-shuffled": _TINY[:30] + (193,) + _TINY[30:],
    "n64": _MANY[:64],
    "n65": _MANY[:65],
    "n66": _MANY[:66],
    "n130": _MANY,
}
POST_N_MAX, POST_F_MAX, POST_SUM_MAX = 130, 256, 3000
# the family of lists the coverage test enumerates inside those limits: m items of a frames then n - m items of b frames
FAMILY_F = (1, 2, 3, 16, 17, 31, 32, 33, 40, 41, 63, 64, 65, 100, 101, 128, 129, 193, 256)


def postnet_family():
    for n in range(2, GEMM_RAGGED_MAX + 1):
        for a in FAMILY_F:
            for b in FAMILY_F:
                for m in sorted({1, n // 2, n - 1}):
                    if 1 <= m < n and m * a + (n - m) * b <= POST_SUM_MAX:
                        yield (a,) * m + (b,) * (n - m)


# A class of the enumerated space that no case reaches stays out only with its reason here.
LEFT_OUT = {}
# A case that is the only one of no class is kept only with its reason here (test_batch_shapes_cpu.py asserts both).
ENCODER_KEPT = {
    (2, 1): "the smallest batch there is: every site split with two items of one row, item 1 the last block of the grid",
    (17, 1): "the first batch whose convolutions are not split while the memory layer still is: 17 one-row tiles",
    (33, 1): "bilstm_proj on 64x64 tiles of one row each under the plain mapping (the class is shared with (65, 1) alone)",
    (2, 65): "memory under the XCD mapping with the fewest items: 6 row tiles, the item boundary in the only, padded group",
    (4, 33): "memory under the XCD mapping with exactly one full group of 8 holding four items of two tiles, the second one row high",
    (16, 65): "bilstm_proj on 64x64 tiles under the XCD mapping while the convolutions still run 32x32 unsplit and plain",
    (40, 65): "all three sites XCD-mapped with every group full: 80 tiles of 64 (the last of each item one row high) and 120 of 32",
    (41, 65): "the same with one chunk more: every site's last group padded at once",
}
POSTNET_KEPT = {
    "five": "five items in shuffled order, each of another length, all split four ways: the pair of five-longest-first",
    "five-longest-first": "the same five items in the order the batched decode leaves them: column offsets permuted against `five`",
    "tiles12-s2": "layers 1-3 at two slices with equal items (no early return), and the longer list of the call-order test",
    "tiles17-s1": "the first tile count at which layers 1-3 are not split while layer 4 still runs four slices; ends in a one-frame item",
    "sum400": "the last frame total at which layer 4 keeps the plain mapping and its four slices",
    "sum401": "the first frame total at which layer 4 goes to the XCD mapping: 16 row tiles, two full groups of 8",
    "sum438-short": "layer 4 XCD-mapped with full groups that hold one-frame items beside a 193-frame one",
    "n50-sum2560": "the last frame total at which layers 0-3 keep the plain mapping at 50 items on 32x32 tiles",
    "n50-sum2561": "the first frame total past it: layers 0-3 XCD-mapped on 32x32 tiles, the last group padded",
    "n64-sum2560": "64 items, so 64x64 tiles (8 x 1 x 64 = 512 tiles of 64), at the last frame total of the plain mapping",
    "n64-one-long": "layer 4 `big` because of one long item: 63 of its 67 row tiles of 64 hold one to three rows; longest first",
    "n64-one-long-shuffled": "the same items with the long one in the middle: tile_id and column offsets of the items behind it move",
    "n64": "exactly one full group of GEMM_RAGGED_MAX items",
    "n65": "a second group of one item: it must land at its own column offset and take its residual from its own frames",
    "n66": "a second group of two items: the smallest ragged launch behind a full one, zero buffers re-filled for its layout",
}

# call order (test_gpu_encoder_batch_shapes.py): ("enc", B, T, engine) / ("enc1", T) / ("post", case, per_chunk) / ("post1", F)
ORDER = (
    ("post", "tiles12-s2", False), ("enc", 24, 48, None), ("post1", 40), ("enc", 22, 48, None), ("post", "sum401", True),
    ("enc1", 48), ("post", "n64-one-long", False), ("post", "n64-one-long-shuffled", False), ("enc", 65, 1, None),
    ("post", "five-longest-first", True), ("enc", 9, 1, None), ("post", "n66", True), ("enc", 4, 33, "single"),
    ("post", "five", False), ("enc1", 1), ("enc", 2, 65, None), ("post", "pair", False), ("enc", 16, 65, "single"),
    ("post", "tiles12-s2", True), ("post", "short-after-long", False), ("enc", 2, 1, None),
)
# the same n and Fmax as "tiles12-s2" with shorter items: rows that list wrote now lie behind these items' ends
ORDER_LISTS = {"short-after-long": (40, 7, 40, 1, 18, 33)}


def postnet_list(name):
    return POSTNET_CASES[name] if name in POSTNET_CASES else ORDER_LISTS[name]


# ---- chunk pools and references ------------------------------------------------------------------------------------------

def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def encoder_chunk(T, k, synth_ids):
    """ids of chunk k of window T: synth_ids seeded by (T, k) with a first id that differs between any two chunks of a pool
    (synth_ids alone ends every chunk in '.', so all chunks of T = 1 would be one); every third chunk has a zero-padded tail."""
    valid = T if k % 3 != 2 or T < 2 else 1 + (5 * k + 3) % (T - 1)
    ids = np.zeros(T, dtype=np.int64)
    ids[:valid] = synth_ids(valid + 6, seed=1000 * T + k)[:valid]
    ids[0] = 64 + (37 * k + T) % 84
    return ids


_ENC = {}
SPENT = {"encoder": 0.0, "postnet": 0.0, "encoder_rows": 0, "postnet_frames": 0}


def encoder_ref(orc, orc64, blob, T, k, synth_ids):
    """ids, fp64 memory and processed_memory of chunk k of window T, d32 of each (the worst row)."""
    if (T, k) not in _ENC:
        t0 = time.time()
        ids = encoder_chunk(T, k, synth_ids)
        m64, p64 = orc64.encoder(blob, ids)
        m32, p32 = orc.encoder(blob, ids)
        _ENC[(T, k)] = _frozen(ids, m64, p64) + (gs.worst(m32, m64, 1), gs.worst(p32, p64, 1))
        SPENT["encoder"] += time.time() - t0
        SPENT["encoder_rows"] += T
    return _ENC[(T, k)]


def postnet_chunk(F, k):
    """(F, 80) standard-normal frames of chunk k of length F."""
    return np.random.default_rng([SEED, F, k]).standard_normal((F, gs.N_MEL)).astype(np.float32)


_POST = {}


def postnet_ref(orc, orc64, blob, F, k):
    """frames, the fp64 oracle's contribution of the stack (out - frames^T, (80, F)) and d32 on it (the worst frame)."""
    if (F, k) not in _POST:
        t0 = time.time()
        fr = postnet_chunk(F, k)
        c64 = orc64.postnet(blob, fr) - fr.T.astype(np.float64)
        c32 = orc.postnet(blob, fr).astype(np.float64) - fr.T.astype(np.float64)
        _POST[(F, k)] = _frozen(fr, c64) + (gs.worst(c32, c64, 0),)
        SPENT["postnet"] += time.time() - t0
        SPENT["postnet_frames"] += F
    return _POST[(F, k)]


def list_items(Fs):
    """(F, k) of every item of a list: the i-th item of length F in the list is chunk i of that length's pool."""
    seen, out = {}, []
    for F in Fs:
        out.append((F, seen.get(F, 0)))
        seen[F] = out[-1][1] + 1
    return out


def prime(fn, keys, workers=4):
    """fn(*key) of many keys on a few threads (the oracle runs outside the interpreter lock)."""
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(lambda k: fn(*k), keys))


def encoder_keys(G=G_MI355X):
    pool = {}
    for B, T in ENCODER_CASES + tuple((B, T) for B, _ in bilstm_batches(G).values() for T in BILSTM_T):
        pool[T] = max(pool.get(T, 0), B)
    return [(T, k) for T, n in sorted(pool.items()) for k in range(n)]


def postnet_keys():
    return sorted({it for Fs in POSTNET_CASES.values() for it in list_items(Fs)})


# ---- one GPU case: run, print the figures and their yardsticks, assert --------------------------------------------------------

def check_encoder(model, orc, orc64, blob, synth_ids, B, T, engine, record, tag, classes):
    """encoder_batch of the first B chunks of window T against each chunk's own references, every row of both outputs."""
    refs = [encoder_ref(orc, orc64, blob, T, k, synth_ids) for k in range(B)]
    t0 = time.time()
    mem, pm = model.encoder_batch(np.stack([r[0] for r in refs]), engine=engine)
    dt = time.time() - t0
    assert mem.shape == (B, T, 512) and pm.shape == (B, T, 128) and np.all(np.isfinite(mem)) and np.all(np.isfinite(pm)), (B, T, engine)
    worst, fails = {}, []
    for b, (ids, m64, p64, dm, dp) in enumerate(refs):
        for name, got, ref, d32 in (("memory", mem[b], m64, dm), ("processed_memory", pm[b], p64, dp)):
            rows = gs.per_row_rel(got, ref, 1)
            e = float(rows.max())
            w = (e / gs.bound(d32), e, d32, b, int(np.argmax(rows)))
            if name not in worst or w > worst[name]:
                worst[name] = w
            if e > gs.bound(d32):
                fails.append((name, b, w[4], e, d32))
    wm, wp = worst["memory"], worst["processed_memory"]
    print("batch-shapes %-8s B=%2d T=%3d engine=%-11s memory err(gpu,f64) %.2e d32 %.2e bound %.2e (chunk %d row %d) | processed_memory %.2e d32 %.2e "
          "bound %.2e (chunk %d row %d)  %.0f ms  %s" % (tag, B, T, engine, wm[1], wm[2], gs.bound(wm[2]), wm[3], wm[4], wp[1], wp[2], gs.bound(wp[2]),
                                                        wp[3], wp[4], 1e3 * dt, " ".join(sorted(classes))), flush=True)
    record("%s/B%d/T%d/%s" % (tag, B, T, engine), {n: {"err": w[1], "d32": w[2], "bound": gs.bound(w[2]), "chunk": w[3], "row": w[4]} for n, w in worst.items()})
    assert not fails, (B, T, engine, fails[:6])
    return mem, pm


def check_postnet(model, orc, orc64, blob, name, record):
    """postnet_batch of a list in both layouts: bit-equal to each other, every frame of every item within its item's bound."""
    Fs = postnet_list(name)
    refs = [postnet_ref(orc, orc64, blob, F, k) for F, k in list_items(Fs)]
    frames = [r[0] for r in refs]
    t0 = time.time()
    wide = model.postnet_batch(frames, per_chunk=False)
    dense = model.postnet_batch(frames, per_chunk=True)
    dt = time.time() - t0
    assert wide.shape == (gs.N_MEL, sum(Fs)) and wide.dtype == np.float32 and np.all(np.isfinite(wide)), name
    assert len(dense) == len(Fs) and all(d.shape == (gs.N_MEL, F) for d, F in zip(dense, Fs)), name
    worst, fails, off = None, [], 0
    for i, (F, (fr, c64, d32)) in enumerate(zip(Fs, refs)):
        part = wide[:, off:off + F]
        if not np.array_equal(part, dense[i]):
            fails.append(("layouts differ", i, F, float(np.abs(part - dense[i]).max())))
        cols = gs.per_row_rel(part.astype(np.float64) - fr.T.astype(np.float64), c64, 0)
        e = float(cols.max())
        w = (e / gs.bound(d32), e, d32, i, F, int(np.argmax(cols)))
        worst = w if worst is None or w > worst else worst
        if e > gs.bound(d32):
            fails.append(("bound", i, F, w[5], e, d32))
        off += F
    print("batch-shapes postnet  %-22s n=%3d sum F=%4d err(gpu,f64) %.2e d32 %.2e bound %.2e (item %d of %d frames, frame %d)  %.0f ms  %s" % (
        name, len(Fs), sum(Fs), worst[1], worst[2], gs.bound(worst[2]), worst[3], worst[4], worst[5], 1e3 * dt, " ".join(sorted(postnet_classes(Fs)))), flush=True)
    record("postnet/%s" % name, {"err": worst[1], "d32": worst[2], "bound": gs.bound(worst[2]), "item": worst[3], "frames": worst[4], "frame": worst[5]})
    assert not fails, (name, fails[:6])
    return wide
