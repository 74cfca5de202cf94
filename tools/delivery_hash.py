"""Developer aid: the bits of everything the vocoder's delivery chain delivers (delivery.cpp: output rate -> compressor -> output
normalisation | loudness -> limiter, and the stream stage behind it), as one line per delivered array -- sha1 of its bytes, then
the fields of the stats structs of the call, floats as exact hex -- for a fixed list of calls under three settings: every stage off, every stage on at
8000 Hz, every stage on at 48000 Hz.  Two builds of the library deliver the same bits exactly when their outputs are equal line
for line (XDTTS_LIB selects the build):

  python tools/delivery_hash.py > new.txt
  XDTTS_LIB=path/to/other/libxdtts_hip.so python tools/delivery_hash.py > old.txt && diff old.txt new.txt

The calls: a single infer; a ragged infer_batch of five; one synthesize_sequence of three utterances over the small golden model
(tests/golden/tacotron2_small.npz: its weight seed, and its ids as the first utterance); one synthesize_document of the same in
PCM16, at level 0 and at programme level."""
import hashlib, importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (one HIP runtime per process: torch's first)
pkg = importlib.import_module("xd-tts_amd")
wl = importlib.import_module("xd-tts_amd.workloads")

FRAMES = (40, 2, 17, 123, 18)  # the ragged five: several compressor tiles, below one, exactly one, an odd many, just over one
GAPS = (0, 441, 0, 100)
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "tacotron2_small.npz"))


def mel(rng, F):
    return (rng.uniform(-7.0, -1.0, size=(80, F)) + 1.5 * np.sin(np.arange(F) / 4.0)[None, :]).astype(np.float32)


def fields(s):
    """every field of a stats struct, floats as their exact hex (the padding between fields is not part of the result)"""
    vals = [getattr(s, name) for name, _ in s._fields_]
    return "/".join(x.hex() if isinstance(x, float) else str(x) for x in vals)


def stats(voc):
    return " ".join("%s=[%s]" % (name, ",".join(fields(s) for s in got))
                    for name, got in (("loud", voc.last_loudness()), ("lim", voc.last_limiter()), ("comp", voc.last_compressor())))


def line(tag, a, voc):
    a = np.ascontiguousarray(a)
    print("%-28s %s n=%-7d %s %s" % (tag, a.dtype, a.size, hashlib.sha1(a.tobytes()).hexdigest(), stats(voc)))


def run(setting, rate, model):
    voc = pkg.create_griffin_lim(iters=4, seed=5)
    if rate:
        voc.set_output_rate(rate)
        voc.set_compressor(pkg.compressor_preset(1))
        voc.set_loudness(-23.0, -1.0)
        voc.set_limiter(5000)
    rng = np.random.default_rng(20)
    mels = [mel(rng, F) for F in FRAMES]
    line("%s single" % setting, voc.infer(mels[0]), voc)
    for u, a in enumerate(voc.infer_batch(mels)):
        line("%s batch[%d]" % (setting, u), a, voc)
    ids = [GOLDEN["ids"].astype(np.int64)] + [wl.synth_ids(n, seed=71 + i) for i, n in enumerate([33, 52])]
    o = pkg.default_opts(fixed_frames_per_id=2.0, dropout_seed=2)
    _m, audios = pkg.synthesize_sequence(model, voc, ids, None, opts=o, want_mels=False)
    for u, a in enumerate(audios):
        line("%s sequence[%d]" % (setting, u), a, voc)
    for level in (0, 1) if rate else (0,):  # (programme level needs a loudness target)
        _m, pcm, off = pkg.synthesize_document(model, voc, ids, GAPS, pkg.StreamOpts(format=1, level=level), opts=o, want_mels=False)
        line("%s document level %d" % (setting, level), pcm, voc)
        print("%-28s offsets %s" % ("", list(off)))
    voc.close()


def main():
    if pkg.device_count() < 1:
        sys.exit("delivery_hash.py needs a HIP device")
    model = pkg.Tacotron2.synthetic(seed=int(GOLDEN["weight_seed"]))
    for setting, rate in (("off", 0), ("on@8000", 8000), ("on@48000", 48000)):
        run(setting, rate, model)
    model.close()


if __name__ == "__main__":
    main()
