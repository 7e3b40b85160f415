"""Which (layer, head) of FlowLM aligns with the text: for operators who have
the real checkpoint. Runs a few texts once per layer and head (one head per run, then the full mask)
on an align-enabled engine, collects each run's frames x tokens matrix (Engine.fetch_align) and ranks
the (layer, head) pairs by align.diagonality, the mean over the texts.

On synthetic weights (no --weights) every softmax over the text is almost flat, all scores sit near
1 / tokens and the ranking means nothing: the tool says so and still prints it.

python tools/align_heads.py --tokenizer tokenizer.model [--weights model.safetensors] [--layers 0,1,..]
                            [--heads 0,1,..] [--frames N] [text ...]"""
import argparse
import statistics
import sys

import numpy as np

sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1] / "pocket-tts_amd"))
import pocket_tts_amd as pt  # noqa: E402
from pocket_tts_amd import align  # noqa: E402

TEXTS = ["The quick brown fox jumps over the lazy dog.",
         "She sells sea shells by the sea shore, and the shells she sells are sea shells.",
         "Timestamps say when each word is spoken."]


def matrix(layer, mask, ids, prompt, args):
    eng = pt.Engine(device=0, max_slots=1, max_ctx=prompt.shape[0] + len(ids) + args.frames + 8, lsd_decode_steps=1,
                    seed=0x5EED, weights_path=args.weights, align=True, align_layer=layer, align_heads=mask)
    try:
        p = pt.GenerationParams(temp=0.0, max_frames=args.frames, seed=1)
        p.align = True
        eng.open(0, eng.voice_from_prompt(prompt), ids, p)
        rows = []
        while True:
            r = eng.step(1)
            if not r.valid[0]:
                break
            rows.append(eng.fetch_align(1)[0])
            if r.last[0]:
                break
        return np.stack(rows) if rows else np.zeros((0, len(ids)))
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tokenizer", required=True)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--layers", default="0,1,2,3,4,5")
    ap.add_argument("--heads", default=",".join(str(h) for h in range(16)))
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--prompt-frames", type=int, default=25)
    ap.add_argument("texts", nargs="*")
    args = ap.parse_args()
    tok = pt.load_tokenizer(args.tokenizer)
    texts = args.texts or TEXTS
    ids = [np.asarray(tok(pt.prepare_text_prompt(t)), np.int32) for t in texts]
    if any(i.size > 128 for i in ids):
        sys.exit("a text has more than 128 tokens (PTTS_ALIGN_TOKENS)")
    prompt = (0.1 * np.random.default_rng(0).standard_normal((args.prompt_frames, 1024))).astype(np.float32)
    if not args.weights:
        print("synthetic weights: the rows are almost flat, this ranking means nothing", flush=True)
    layers = [int(x) for x in args.layers.split(",")]
    masks = [(str(h), 1 << int(h)) for h in args.heads.split(",")] + [("all", 0xFFFF)]
    scores = []
    for layer in layers:
        for name, mask in masks:
            d = [align.diagonality(matrix(layer, mask, i, prompt, args)) for i in ids]
            scores.append((statistics.mean(d), layer, name, d))
            print(f"layer {layer} head {name:>3}: diagonality {scores[-1][0]:.4f}  {[round(x, 4) for x in d]}", flush=True)
    print("ranking (layer, head, mean diagonality):")
    for s, layer, name, _ in sorted(scores, reverse=True):
        print(f"  {layer}  {name:>3}  {s:.4f}")


if __name__ == "__main__":
    main()
