"""The stream stage (document output: a sequence joined with its breaks as fp32 / PCM16 / G.711 on the device, DESIGN.md
section 4.11) through the product alone.
  stage alone   k_stream_join through xdtts_griffinlim_join (HIP events on the handle's stream, best / median of 20) at the
                headline utterance's 204 544 samples and at 8 x that, in each format, next to the traffic floor -- one read of the
                fp32 signal, one write of 4, 2 or 1 bytes a sample, over the achievable HBM rate -- and next to a one-sample
                call, the launch floor.
  end to end    eight headline utterances with 0.25 s gaps to PCM16 as ONE xdtts_synthesize_document call, against what a host
                does without it: xdtts_synthesize_sequence + xdtts_audio_to_i16 + the memcpy join, in the same process (wall
                clock, best / median of 20, alternating), with the bytes each form moves over PCIe.

  python tools/document_check.py                       # prints the table
  python tools/document_check.py > profiles/document.txt
  python tools/document_check.py 2                     # fewer repetitions (tools/selftest.sh)
"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (one HIP runtime per process: torch's first)
pkg = importlib.import_module("xd-tts_amd")
wl = importlib.import_module("xd-tts_amd.workloads")

HBM_BYTES_PER_S = 6.3e12  # achievable (float4 copy), of 8 TB/s peak
N_HEADLINE = 204544
NAMES = {0: "fp32", 1: "PCM16", 2: "mu-law", 3: "A-law"}


def stage_us(voc, audios, gaps, opts, n):
    voc.join(audios, gaps, opts=opts)  # warm: buffers, code object
    us = []
    for _ in range(n):
        voc.join(audios, gaps, opts=opts)
        us.append(voc.last_timings()["mel_to_linear_ms"] * 1e3)
    return min(us), float(np.median(us))


def stage(voc, reps):
    print("device time of k_stream_join alone (xdtts_griffinlim_join, HIP events, best / median of %d):" % reps)
    for mult in (1, 8):
        audios = [wl.chirps(N_HEADLINE) for _ in range(mult)]
        gaps = [0] + [5513] * (mult - 1) + [0]
        total = mult * N_HEADLINE + 5513 * (mult - 1)
        for fmt in (0, 1, 2, 3):
            sb = pkg.stream_sample_bytes(fmt)
            floor = (mult * N_HEADLINE * 4 + total * sb) / HBM_BYTES_PER_S * 1e6
            best, med = stage_us(voc, audios, gaps, pkg.StreamOpts(format=fmt), reps)
            one, one_med = stage_us(voc, [audios[0][:1]], None, pkg.StreamOpts(format=fmt), reps)
            print("  %d x %d samples (+ gaps = %7d)  %-6s  %6.1f us (median %6.1f)   traffic floor (1 read + 1 write of %d B) %5.2f us"
                  "   one-sample call %5.1f us (median %5.1f)" % (mult, N_HEADLINE, total, NAMES[fmt], best, med, sb, floor, one, one_med))


def end_to_end(reps):
    model = pkg.Tacotron2.synthetic(seed=wl.WEIGHT_SEED)
    voc = pkg.create_griffin_lim(iters=60, seed=0)
    _ids, chunks, _steps = wl.config2(pkg)
    sp = np.cumsum([len(c) for c in chunks]).astype(np.uintp)
    utts = [wl.synth_ids(120, seed=1 + g) for g in range(8)]
    o = pkg.default_opts(fixed_frames_per_id=wl.FRAMES_PER_ID, dropout_seed=0, item_base=0)
    gap = pkg.silence_samples(0.25)
    gaps = [0] + [gap] * 7 + [0]

    def host_join():
        _m, audios = pkg.synthesize_sequence(model, voc, utts, [sp] * 8, opts=o, want_mels=False)
        pcm = [pkg.audio_to_i16(a) for a in audios]
        out = np.zeros(sum(p.size for p in pcm) + sum(gaps), np.int16)
        at = gaps[0]
        for p, g in zip(pcm, gaps[1:]):
            out[at:at + p.size] = p
            at += p.size + g
        return out, sum(a.size for a in audios) * 4

    def document():
        _m, stream, _off = pkg.synthesize_document(model, voc, utts, gaps, pkg.StreamOpts(format=1), [sp] * 8, opts=o, want_mels=False)
        return stream, stream.size * 2

    for _ in range(2):
        a, bytes_a = host_join()
        b, bytes_b = document()
    assert np.array_equal(a, np.asarray(b)), "the document is not the host's join"
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); host_join(); ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); document(); tb.append(time.perf_counter() - t0)
    print("eight headline utterances (120 ids -> 800 frames, 60 iterations) with 0.25 s gaps to PCM16, wall clock, best / median of %d, alternating:" % reps)
    print("  xdtts_synthesize_sequence + xdtts_audio_to_i16 + memcpy join   %8.3f ms (median %8.3f)   audio over PCIe %8d B" % (min(ta) * 1e3, np.median(ta) * 1e3, bytes_a))
    print("  xdtts_synthesize_document                                      %8.3f ms (median %8.3f)   audio over PCIe %8d B" % (min(tb) * 1e3, np.median(tb) * 1e3, bytes_b))
    print("  (same bytes: the two streams are equal)")
    voc.close()
    model.close()


if __name__ == "__main__":
    if pkg.device_count() < 1:
        sys.exit("document_check.py needs a HIP device: nothing here is measured without one")
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    voc = pkg.create_griffin_lim(iters=8, seed=3)
    stage(voc, reps)
    voc.close()
    end_to_end(reps)
