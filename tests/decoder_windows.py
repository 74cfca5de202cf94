"""Shared by test_decoder_windows_cpu.py and test_gpu_decoder_windows.py: what every decoder engine does with the encoder
window T restated in plain Python, the windows that reach every shape class of that restatement, the n_valid of every chunk,
a crafted decoder state on which one lost window element shows, the per-position metric, mutations of an oracle step that
imitate a wrong kernel, and the references (fp64 oracle, and the fp32 oracle's own distance from it), computed once.

The rules restated here (csrc/decoder.hip, csrc/decoder_persistent*.hip, csrc/tacotron2_handle.cpp):

  batched engine   location features: T <= LOC_MFMA_T = 128 location_chunk_mfma (16-step tiles, MT = ceil(T / 16), two blocks per
                   chunk: tiles 0..3 and 4..7), else location_blocks (8-step tiles, a block takes eight of them in two rounds of
                   four, loc_blocks_per_chunk = ceil(ceil(T / 8) / 8) = 3..8 blocks).
                   attention_chunk<NT>: energies of steps lane + 64 u, u < 2, from prefetched registers, then
                   `for (t = lane + 128; t < T; t += 64)`; publish / gather / write-back `for (t = tid; t < T; t += NT)` with
                   `t == tid ? awc_pre : awc_in[t]`; NT = 512 inside the attention-LSTM launch (XDTTS_ATT_FUSED=2, the default),
                   256 as k_attention_b (1) and as k_softmax_ctx (0); the context loop `for (t0 = tg; t0 < T; t0 += 16 * 7)`
                   takes its first round from prefetched registers; the prenet rides as the tail of the decoder-LSTM launch
                   (two-launch form) for T <= PERSIST_T_MAX = 128 unless XDTTS_NO_TAIL.
  launch engine    location_tile: 8-step tiles, one block each, a window of 8 + 2 x 15 zero-padded steps, the dense role's two
                   halves take 4 steps each; k_softmax_ctx: 256 threads, `for (t = tid + 256; t < T; t += 256)`, the same
                   context loop.
  persistent       (decoder_persistent.hip, decoder_persistent8.hip, decoder_persistent16.hip; T <= TP = 128): lane l keeps the
                   attention weights of steps l and l + 64; the location role runs all eight 16-row MFMA tiles over a window
                   zero-padded to WPAD = TP + 32, of which ceil(T / 16) hold weights; energies cross in rows of EP_LD = 128.
"""
import numpy as np

T_MAX = 512           # csrc/common.h
PERSIST_T_MAX = 128   # csrc/kernels.h (TP of the persistent kernels)
LOC_MFMA_T = 128      # csrc/decoder.hip
LOC_TT = 8            # csrc/decoder.hip
LOC_K = 31            # csrc/common.h: 15 steps of padding either side
CTX_ROUND = 16 * 7    # TG * CTX_PF rows of the context loop per round
ENGINE_T_MAX = {"launch": T_MAX, "persistent": PERSIST_T_MAX, "batched": T_MAX, "persistent8": PERSIST_T_MAX}
# the positions either side of which a window class changes: the extra weight of crafted_state and the drops of MUTATIONS sit there
CLASS_EDGES = (15, 16, 63, 64, 127, 128, 255, 256)


def cdiv(a, b):
    return -(-a // b)


def loc_blocks_per_chunk(T):
    return (cdiv(T, LOC_TT) + 7) // 8


def _ctx_classes(T):
    return {"ctx:prefetch-only" if T <= CTX_ROUND else "ctx:prefetch+memory",
            "ctx:last-round-%s" % ("full" if T % CTX_ROUND == 0 else "partial")}


def classes(engine, T, att_fused=2, no_tail=False):
    """The shape classes engine `engine` takes at window T, each a string; a sweep has to reach every string once.
    att_fused / no_tail: the batched engine's attention form (XDTTS_ATT_FUSED, XDTTS_NO_TAIL of the handle)."""
    assert 1 <= T <= ENGINE_T_MAX[engine], (engine, T)
    c = set()
    if engine in ("persistent", "persistent8"):
        c.add("slots:0+1" if T > 64 else "slots:0")                  # lane <-> steps lane, lane + 64
        c.add("tiles16:%d-live" % cdiv(T, 16))                       # of the eight the location role always runs
        c.add("last16:%s" % ("full" if T % 16 == 0 else "partial"))
        c.add("window:%s" % ("TP" if T == PERSIST_T_MAX else "<TP"))
        return frozenset(c)
    if engine == "launch":
        tiles, rem = cdiv(T, LOC_TT), T % LOC_TT
        c.add("loc8:%s" % ("one-tile" if tiles == 1 else "tiles"))
        c.add("loc8:last-%s" % ("full" if rem == 0 else ("le4" if rem <= 4 else "gt4")))  # le4: the second dense half idles
        # a tile whose 8 + 30-step window needs no padding: t0 >= 15 and t0 + 8 + 15 <= T
        c.add("loc8:%s" % ("interior-tile" if any(8 * k >= 15 and 8 * k + 23 <= T for k in range(tiles)) else "all-tiles-padded"))
        c.add("nt256:trips-%d" % cdiv(T, 256))                       # trips-2: `t == tid ? awc_pre : awc_in[t]` takes its second arm
        return frozenset(c | _ctx_classes(T))
    assert engine == "batched"
    nt = 512 if att_fused == 2 else 256
    if T <= LOC_MFMA_T:
        mt = cdiv(T, 16)
        c.add("loc:mfma")
        c.add("mfma16:%d-tiles" % mt)
        c.add("mfma16:last-%s" % ("full" if T % 16 == 0 else "partial"))
        c.add("mfma16:%s" % ("both-halves" if mt > 4 else "second-block-idle"))  # two blocks per chunk, split at step 64
    else:
        tiles, rem = cdiv(T, LOC_TT), T % LOC_TT
        c.add("loc:fma")
        c.add("fma8:%d-blocks" % loc_blocks_per_chunk(T))
        c.add("fma8:last-tile-%s" % ("full" if rem == 0 else ("le4" if rem <= 4 else "gt4")))
        left = tiles % 8  # tiles of the chunk's last block: two rounds of four
        c.add("fma8:last-block-%s" % ("full" if left == 0 else ("round0-partial" if left < 4 else ("round0-only" if left == 4 else "round1-partial"))))
    c.add("energy:%s" % ("slot0" if T <= 64 else "slot0+1"))
    trips = cdiv(max(T - 128, 0), 64)
    c.add("energy:strided-%s" % (trips if trips < 2 else "2+"))
    c.add("nt%d:trips-%d" % (nt, cdiv(T, nt)))
    if att_fused == 2:
        c.add("tail:%s" % ("on" if T <= PERSIST_T_MAX and not no_tail else "off"))
    return frozenset(c | _ctx_classes(T))


def all_classes(engine, **kw):
    out = set()
    for T in range(1, ENGINE_T_MAX[engine] + 1):
        out |= classes(engine, T, **kw)
    return out


# ---- the sweeps ----------------------------------------------------------------------------------------------------
# A window that reaches no class of its own is kept only with its reason here (test_decoder_windows_cpu.py asserts both).
JUSTIFIED = {
    1: "the smallest window: a softmax over one position, every lane but one of every loop idle, T - 1 = 0",
    15: "the last position before the first 16-step tile fills: lane 15 of an A fragment is the chunk's last row",
    16: "the first 16-row tile exactly full and nothing behind it",
    64: "slot 0 exactly full: the last window before `tt + 64 h < T` admits a position of slot 1",
    63: "slot 0 one short of full: lane 63 holds the last position and slot 1 stays empty",
    100: "the reference's own window, the one every other test of the suite runs",
    112: "the context loop's prefetched round exactly full and no row taken from memory",
    128: "the last window of the matrix-core location features, of the tail form and of the persistent kernels (T == TP)",
    192: "the first trip of the strided energy loop exactly full, the location blocks' last block full",
    512: "T_MAX: every array of the window at its full length",
    127: "TP - 1: the last lane of slot 1 is masked by `t + 64 < T`, the energy rows of EP_LD = 128 one short",
    129: "the first window on the FMA location blocks and without the tail form, one step into the strided energy loop",
    193: "the first window whose strided energy loop makes a second trip",
    257: "the first window past the 256-thread stride: one position takes the second arm of `t == tid ? awc_pre : awc_in[t]`",
    511: "T_MAX - 1: every `t < T` guard one short of the arrays' length",
}
SWEEP_PERSISTENT = (1, 15, 16, 17, 33, 63, 64, 65, 81, 100, 127, 128)
SWEEP_WIDE = SWEEP_PERSISTENT + (112, 129, 192, 193, 224, 257, 336, 432, 511, 512)
SWEEPS = {"launch": SWEEP_WIDE, "persistent": SWEEP_PERSISTENT, "batched": SWEEP_WIDE, "persistent8": SWEEP_PERSISTENT}
# the windows of the three-step test: where the second and third step take their location features from inside the loop
STEPS3_PERSISTENT = (16, 64, 65, 100, 128)
STEPS3_WIDE = STEPS3_PERSISTENT + (129, 193, 257, 336, 512)
STEPS3 = {"launch": STEPS3_WIDE, "persistent": STEPS3_PERSISTENT, "batched": STEPS3_WIDE, "persistent8": STEPS3_PERSISTENT}
FORMS_T = (16, 100, 128, 129, 257, 512)  # the batched engine's other attention forms
ENGINES = (("launch", 1), ("launch", 3), ("persistent", 1), ("persistent", 2), ("persistent8", 3), ("persistent8", 8), ("persistent8", 9),
           ("persistent8", 16), ("batched", 1), ("batched", 6), ("batched", 17))
POOL = 17       # chunks per window; a batch of B takes the first B of them
STEP0 = 4
SEED = 20240327
ITEM_BASE = 3
DROPOUT_SEED = 11


def second_step0(T):
    """A third of the windows run again from step 5: the other dropout counter and the other ping-pong half."""
    return T % 3 == 1


def n_valid_pool(T):
    """n_valid of the POOL chunks of window T: T, 1, T - 1, then the class edges below T (64, 65, 16 k, 16 k +- 1, the context
    round and the strides either side), nearest to T first; short windows repeat."""
    edges = []
    for e in (64, 65, 63, 128, 129, 127, 256, 257, 255, 300, 112, 113, 16, 17, 15, 111, 192, 193, 32, 33, 31, 48, 49, 47, 8, 9, 7):
        if 1 < e < T - 1 and e not in edges:
            edges.append(e)
    near = sorted((e for e in {16 * k + d for k in range(1, 33) for d in (-1, 0, 1)} if 1 < e < T - 1 and e not in edges), reverse=True)
    rest = edges + near
    out = [T, 1, max(T - 1, 1)]
    i = 0
    while len(out) < POOL:
        out.append(rest[i % len(rest)] if rest else max(1, T // 2))
        i += 1
    return out


def batch_chunks(B, step0=STEP0, n_steps=1):
    """Pool indices of a batch of B.  Two chunks cannot hold T, 1 and T - 1 at once: the pair takes (T, 1) from step 4,
    (T - 1, T) from step 5 and (T - 1, 1) in the three-step test."""
    if B == 2:
        return (2, 1) if n_steps > 1 else ((0, 1) if step0 == STEP0 else (2, 0))
    return tuple(range(B))


# ---- inputs and the crafted state -----------------------------------------------------------------------------------

NAMES = {"attention_hidden": "att_h", "attention_cell": "att_c", "decoder_hidden": "dec_h", "decoder_cell": "dec_c",
         "attention_weights": "aw", "attention_weights_cum": "awc", "attention_context": "ctx"}
OUTPUTS = tuple(NAMES) + ("decoder_output", "gate_prediction")


def window_inputs(T, chunk):
    """memory (T, 512) and processed memory (T, 128) of one chunk: standard normal x 0.5."""
    rng = np.random.default_rng([SEED, T, chunk])
    mem = (rng.standard_normal((T, 512)) * 0.5).astype(np.float32)
    pm = (rng.standard_normal((T, 128)) * 0.5).astype(np.float32)
    return mem, pm


def _field(state, name):
    return np.ctypeslib.as_array(getattr(state, name))


def crafted_state(oracle, T, n_valid, memory, seed):
    """An oracle State in which no window position is negligible: a non-uniform previous alignment with extra weight on the
    first and last valid position and on every class edge, a cumulative alignment three times as large, the context those
    weights give (the persistent engine works from the weights and refuses any other), LSTM vectors of N(0, 0.3) and a
    standard-normal decoder input."""
    rng = np.random.default_rng([SEED, seed])
    a = rng.random(n_valid) + 0.05
    for p in {0, n_valid - 1} | {e for e in CLASS_EDGES if e < n_valid}:
        a[p] += 3.0
    a = a.astype(np.float32)
    a = a / a.sum(dtype=np.float32)
    cum = (3.0 * a + 0.01 * rng.random(n_valid)).astype(np.float32)
    st = oracle.new_state()
    for name in ("att_h", "att_c", "dec_h", "dec_c"):
        _field(st, name)[:] = rng.standard_normal(1024) * 0.3
    _field(st, "dec_in")[:] = rng.standard_normal(80)
    _field(st, "aw")[:] = 0.0
    _field(st, "awc")[:] = 0.0
    _field(st, "aw")[:n_valid] = a
    _field(st, "awc")[:n_valid] = cum
    _field(st, "ctx")[:] = (a.astype(np.float64) @ np.asarray(memory[:n_valid], dtype=np.float64)).astype(np.float32)
    # every value is a float32, whichever precision the struct has
    for name in ("att_h", "att_c", "dec_h", "dec_c", "dec_in"):
        _field(st, name)[:] = _field(st, name).astype(np.float32)
    return st


def copy_state(dst, src):
    """an oracle state into another struct (of either precision)"""
    for v in tuple(NAMES.values()) + ("dec_in",):
        _field(dst, v)[:] = _field(src, v)
    return dst


def snapshot(state, T):
    """One state as float32 arrays under the reference's tensor names, plus decoder_input."""
    out = {k: np.array(_field(state, v), dtype=np.float32)[: (T if v in ("aw", "awc") else None)] for k, v in NAMES.items()}
    out["decoder_input"] = np.array(_field(state, "dec_in"), dtype=np.float32)
    return out


def run_steps(oracle, blob, mem, pm, n_valid, state, item, step0, n_steps):
    """n_steps oracle steps from `state` (advanced in place): the nine outputs, the frames and gate logits stacked."""
    T = mem.shape[0]
    opts = oracle.default_opts(dropout_seed=DROPOUT_SEED, item=item)
    frames, gates = np.zeros((n_steps, 80), dtype=np.float64), np.zeros(n_steps, dtype=np.float64)
    for i in range(n_steps):
        frames[i], gates[i] = oracle.decoder_step(blob, mem, pm, n_valid, state, opts, step0 + i)
    out = {k: np.array(_field(state, v), dtype=np.float64)[: (T if v in ("aw", "awc") else None)] for k, v in NAMES.items()}
    out["decoder_output"] = frames
    out["gate_prediction"] = gates
    return out


# ---- the metric -----------------------------------------------------------------------------------------------------

def errors(got, ref64, n_valid):
    """One chunk's nine outputs against the fp64 oracle's: the alignment position by position, |got / ref - 1| over the valid
    ones (a softmax weight never vanishes there), every other output max|got - ref| / max(1, |ref|_inf)."""
    e = {}
    for k in OUTPUTS:
        g, r = np.asarray(got[k], dtype=np.float64), np.asarray(ref64[k], dtype=np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if k == "attention_weights":
            e[k] = float(np.abs(g[:n_valid] / r[:n_valid] - 1.0).max())
        else:
            e[k] = float(np.abs(g - r).max() / max(1.0, float(np.abs(r).max())))
    return e


def bound(d32, extra=1e-6):
    """err(gpu, f64) <= 4 d32 + 1e-6, d32 = the fp32 oracle's distance from the fp64 oracle in the same metric at the same case."""
    return 4.0 * d32 + extra


def masked_is_zero(got, n_valid):
    return bool(np.all(np.asarray(got["attention_weights"])[n_valid:] == 0.0) and all(np.all(np.isfinite(np.asarray(got[k]))) for k in OUTPUTS))


# ---- references, computed once per (window, chunk, item, step range) and never modified ------------------------------

_REF = {}


def reference(orc, orc64, blob, T, chunk, item, step0, n_steps):
    """(memory, pmem, n_valid, start: the crafted state as arrays, ref64: the fp64 oracle's outputs, d32: the fp32 oracle's
    errors against them)."""
    key = (T, chunk, item, step0, n_steps)
    if key not in _REF:
        mem, pm = window_inputs(T, chunk)
        nv = n_valid_pool(T)[chunk]
        st32 = crafted_state(orc, T, nv, mem, seed=1000 * T + chunk)
        st64 = copy_state(orc64.new_state(), st32)
        start = snapshot(st32, T)
        r64 = run_steps(orc64, blob, mem, pm, nv, st64, item, step0, n_steps)
        r32 = run_steps(orc, blob, mem, pm, nv, st32, item, step0, n_steps)
        assert masked_is_zero(r32, nv) and masked_is_zero(r64, nv), key
        for a in (mem, pm) + tuple(start.values()) + tuple(r64.values()):
            a.setflags(write=False)
        _REF[key] = (mem, pm, nv, start, r64, errors(r32, r64, nv))
    return _REF[key]


def prime(orc, orc64, blob, keys, workers=4):
    """reference(...) of many (T, chunk, item, step0, n_steps) on a few threads (the oracle's steps run outside the interpreter lock)."""
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(lambda k: reference(orc, orc64, blob, *k), [k for k in keys if k not in _REF]))


# ---- mutations: an oracle step whose inputs are what a wrong kernel would have read ------------------------------------

def _drop(name, pos):
    def f(state, n_valid):
        _field(state, name)[pos(n_valid)] = 0.0
        return n_valid
    return f


def _zero_tile(width):
    def f(state, n_valid):
        t0 = ((n_valid - 1) // width) * width if n_valid < 2 * width else width  # the second tile, or the only / last one
        _field(state, "aw")[t0:t0 + width] = 0.0
        return n_valid
    return f


def _mask_short(state, n_valid):
    return n_valid - 1


def mutations(n_valid):
    """name -> f(state, n_valid) -> n_valid the step is then given; those that fit a window of n_valid positions."""
    m = {"drop-first": _drop("aw", lambda nv: 0), "drop-last": _drop("aw", lambda nv: nv - 1), "drop-first-of-cumulative": _drop("awc", lambda nv: 0)}
    for e in CLASS_EDGES:
        if e < n_valid - 1:
            m["drop-%d" % e] = _drop("aw", lambda nv, e=e: e)
    if n_valid >= 2:
        m["mask-one-short"] = _mask_short
    m["zero-8-tile"] = _zero_tile(8)
    m["zero-16-tile"] = _zero_tile(16)
    return m


def mutated_step(orc64, blob, T, chunk, item, step0, mutate):
    """The fp64 oracle's step of reference(...) with its inputs spoilt by `mutate`."""
    mem, pm = window_inputs(T, chunk)
    nv = n_valid_pool(T)[chunk]
    st = copy_state(orc64.new_state(), crafted_state(orc64, T, nv, mem, seed=1000 * T + chunk))
    nv2 = mutate(st, nv)
    return run_steps(orc64, blob, mem, pm, nv2, st, item, step0, 1)


# ---- one GPU case: run, print the figures and their yardsticks, assert ---------------------------------------------------

def check_case(model, gpu_opts, orc, orc64, blob, engine, B, T, step0, n_steps, record, tag="steps", extra=1e-6, **plan_kw):
    """decoder_steps of `engine` on B crafted chunks of window T against the references, chunk by chunk and output by output;
    record(key, figures) keeps the figures of the chunk closest to its bound."""
    chunks = batch_chunks(B, step0, n_steps)
    refs = [reference(orc, orc64, blob, T, c, ITEM_BASE + b, step0, n_steps) for b, c in enumerate(chunks)]
    mem, pm = np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
    nvs = [r[2] for r in refs]
    start = {k: np.stack([r[3][k] for r in refs]) for k in NAMES}
    dec_in = np.stack([r[3]["decoder_input"] for r in refs])
    out, gate, gst = model.decoder_steps(engine, mem, pm, nvs, start, dec_in, step0, n_steps, opts=gpu_opts)
    wa, wr = None, None  # (err / bound, err, d32, n_valid, output) of the chunk closest to its bound
    fails = []
    for b in range(B):
        got = dict({k: gst[k][b] for k in NAMES}, decoder_output=out[b], gate_prediction=gate[b])
        if not masked_is_zero(got, nvs[b]):
            fails.append((b, nvs[b], "masked positions not exactly 0, or a non-finite output"))
            continue
        e, d32 = errors(got, refs[b][4], nvs[b]), refs[b][5]
        for k in OUTPUTS:
            if e[k] > bound(d32[k], extra):
                fails.append((b, nvs[b], k, e[k], d32[k], bound(d32[k], extra)))
            w = (e[k] / bound(d32[k], extra), e[k], d32[k], nvs[b], k)
            if k == "attention_weights":
                wa = w if wa is None or w > wa else wa
            else:
                wr = w if wr is None or w > wr else wr
    assert wa is not None and wr is not None, (engine, B, T, step0, n_steps, fails[:6])
    wa, wr = wa[1:], wr[1:]
    print("decoder-windows %-6s %-11s B=%2d T=%3d step0=%d n=%d  alignment err(gpu,f64) %.2e d32 %.2e bound %.2e (n_valid %d) | rest %.2e d32 %.2e bound %.2e (%s, n_valid %d)  %s" % (
        tag, engine, B, T, step0, n_steps, wa[0], wa[1], bound(wa[1], extra), wa[2], wr[0], wr[1], bound(wr[1], extra), wr[3], wr[2],
        " ".join(sorted(classes(engine, T, **plan_kw)))), flush=True)
    record("%s/%s%d/T%d/step%d+%d" % (tag, engine, B, T, step0, n_steps), {
        "alignment": {"err": wa[0], "d32": wa[1], "bound": bound(wa[1], extra), "n_valid": wa[2]},
        "rest": {"err": wr[0], "d32": wr[1], "bound": bound(wr[1], extra), "n_valid": wr[2], "output": wr[3]}})
    assert not fails, (engine, B, T, step0, n_steps, fails[:6])
    return wa[0], wr[0]
