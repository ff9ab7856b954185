"""Which entry points of libdpm_hip.so the model layer calls, with which shapes, and what comes back: the record a host-side
refactor of decoder.py / encoder.py is held to (profiles/model_walk_calls.md).

    python scripts/call_trace.py --out A.pt [--tree DIR]     run every scenario with the package found in DIR (default: this
                                                             tree), save the call traces and every returned tensor
    python scripts/call_trace.py --compare A.pt B.pt         one table row per scenario: calls, traces equal, bytes equal

The object `_lib.load()` returns is swapped for a proxy that notes, for every entry point called, its name and the values of its
non-pointer arguments (told apart by the argtypes in `_lib.SIGNATURES`) and forwards the call.  The scenarios and their seeds are
this file's, so two trees run the same code on the same inputs."""
import argparse
import os
import sys
from ctypes import c_void_p

import torch


class Recorder:
    def __init__(self, lib, signatures):
        self._lib, self._sig, self._fns, self.calls = lib, signatures, {}, []

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is None:
            real, types = getattr(self._lib, name), self._sig[name][1]

            def fn(*args):
                self.calls.append((name,) + tuple(a for a, t in zip(args, types) if t is not c_void_p))
                return real(*args)
            self._fns[name] = fn
        return fn


def descriptors(gen, *lead_and_tokens):
    *lead, M = lead_and_tokens
    return torch.cat([torch.rand(*lead, 128, M, generator=gen), 60 * torch.randn(*lead, 3, M, generator=gen)], len(lead)).cuda()


def known_rows(res):
    """registration result rows (B, 20 + 2k): the entries past a pair's inlier count are unspecified -- zero them"""
    res = res.clone()
    for row in res:
        row[20 + int(row[14]):] = 0
    return res


def scenarios():
    from deeppointmap_amd import synthetic
    from deeppointmap_amd.config import default_args
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.weights import init_procedural
    cfg = default_args()
    dec = init_procedural(Decoder(cfg)).cuda()
    dec.graph_min_hits = 0
    gen = torch.Generator().manual_seed(2024)

    def one_pair(M, N, masked=False):
        s, d = descriptors(gen, M), descriptors(gen, N)
        ms = md = None
        if masked:
            ms, md = torch.zeros(1, M, dtype=torch.bool), torch.zeros(1, N, dtype=torch.bool)
            ms[:, M - 20:], md[:, N - 9:] = True, True
            s, d = s[None], d[None]
        return lambda: [v if torch.is_tensor(v) else torch.tensor(v, dtype=torch.float64)
                        for v in dec.registration_forward(s, d, ms, md, num_sample=0.5)]

    def batch(masked):
        s, d = descriptors(gen, 4, 256), descriptors(gen, 4, 256)
        ms = md = None
        if masked:
            ms, md = torch.zeros(4, 256, dtype=torch.bool), torch.zeros(4, 256, dtype=torch.bool)
            ms[:, 236:], md[:, 247:] = True, True

        def run():   # (registration_forward_batch takes no masks: its core does)
            with torch.no_grad():
                return [known_rows(dec._register(s, d, 0.5, masks=(ms, md)) if masked else dec.registration_forward_batch(s, d, 0.5))]
        return run

    def pairs(dedup):
        frames = descriptors(gen, 9, 256)
        src = torch.arange(0, 8, dtype=torch.int32).cuda()

        def run():
            dec.dedup_frames = dedup
            try:
                return [known_rows(dec.registration_forward_pairs(frames, src, src + 1, 0.5))]
            finally:
                dec.dedup_frames = True
        return run

    def loop():
        s, d = descriptors(gen, 3, 256), descriptors(gen, 3, 256)
        return lambda: [dec.loop_detection_forward(s, d)]

    yield "registration_forward eager 256 x 256", one_pair(256, 256)
    yield "registration_forward eager 256 x 128", one_pair(256, 128)
    yield "registration_forward eager 4096 x 256", one_pair(4096, 256)
    yield "registration_forward eager 256 x 128, both masks", one_pair(256, 128, masked=True)
    yield "registration_forward_batch B=4 256 x 256", batch(False)
    yield "registration_forward_batch B=4 256 x 256, masked", batch(True)
    yield "registration_forward_pairs 8 pairs / 9 frames x 256, dedup_frames on", pairs(True)
    yield "registration_forward_pairs 8 pairs / 9 frames x 256, dedup_frames off", pairs(False)
    yield "loop_detection_forward 3 pairs x 256", loop()

    pts, pad = synthetic.frames(2, 20000)
    pad[1, 14000:] = True
    pts, pad = pts.cuda(), pad.cuda()

    def encoder(levels=None, stop_level=None, **knob):
        def run():
            enc = init_procedural(Encoder(cfg)).cuda()
            for k, v in knob.items():
                setattr(enc, k, v)
            if stop_level is not None:
                return enc(pts, pad, resume=enc(pts, pad, stop_level=stop_level))
            return enc(pts, pad, presampled=enc.presample(pts, pad, levels=levels) if levels is not None else None)
        return run

    yield "Encoder.forward", encoder()
    yield "Encoder.forward, presample_neighbours", encoder(presample_neighbours=True)
    yield "Encoder.forward, presample_neighbours_from = 2", encoder(presample_neighbours_from=2)
    yield "Encoder.forward, presample(levels=2)", encoder(levels=2)
    yield "Encoder.forward, stop_level = 2 then resume", encoder(stop_level=2)


def record(out):
    from deeppointmap_amd import _lib
    rec = Recorder(_lib.load(), _lib.SIGNATURES)
    _lib._lib = rec
    torch.set_grad_enabled(False)
    result = {}
    for name, run in scenarios():
        del rec.calls[:]
        tensors = [t.detach().cpu() for t in run()]
        torch.cuda.synchronize()
        result[name] = dict(calls=list(rec.calls), tensors=tensors)
        print(f"{name}: {len(rec.calls)} calls, {len(tensors)} tensors")
    torch.save(result, out)


def compare(a, b):
    A, B = torch.load(a, weights_only=False), torch.load(b, weights_only=False)
    print("| scenario | calls | traces equal | returned bytes equal |\n|---|---|---|---|")
    ok = A.keys() == B.keys()
    for name in A:
        x, y = A[name], B.get(name, dict(calls=None, tensors=[]))
        same_calls = x["calls"] == y["calls"]
        same_bytes = len(x["tensors"]) == len(y["tensors"]) and all(
            s.shape == t.shape and s.dtype == t.dtype and s.numpy().tobytes() == t.numpy().tobytes()
            for s, t in zip(x["tensors"], y["tensors"]))
        ok = ok and same_calls and same_bytes
        print(f"| {name} | {len(x['calls'])} | {'yes' if same_calls else 'NO'} | {'yes' if same_bytes else 'NO'} |")
    return ok


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(0 if compare(*args.compare) else 1)
    sys.path.insert(0, os.path.abspath(args.tree))
    record(args.out)
