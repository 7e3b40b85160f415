"""Word timestamps from the align stage's rows. Pure numpy, host only: this
file is the documented definition of a timestamp.

The engine delivers, with every frame t of a row in the align stage, a[t][j] >= 0 over the row's S
text tokens (sum 1): the attention the FlowLM query of step t paid to token j in one layer, averaged
over a set of heads (Engine.fetch_align). From those rows:

  word_spans      which tokens form which word (a word starts at a piece beginning with U+2581)
  monotonic_path  the word spoken in every frame: the best path that starts at the first word and
                  moves on by at most one word per frame
  word_times      frames -> seconds: a word starts at its first frame, 80 ms a frame, scaled by the
                  request's speed (pitch and volume keep the duration)
  diagonality     a score in [0, 1] of how well a frames x tokens matrix follows such a path
                  (tools/align_heads.py ranks (layer, head) by it)

The resolution is one frame (80 ms). Nothing here judges whether a given layer and head set aligns
on a given checkpoint: on synthetic weights the rows are almost flat and the times mean nothing."""

from __future__ import annotations

import numpy as np

META = "▁"
FRAME_SECONDS = 0.08  # 1920 samples at 24 kHz
FLOOR = 1e-8


def _piece_text(piece: str) -> str:
    return piece.replace(META, "")


def word_spans(tokenizer, ids) -> list[tuple[str, int, int]]:
    """[(word, j0, j1)]: tokens j0 .. j1 - 1 of the encoding `ids` spell `word`. A word starts at a
    piece beginning with U+2581 (and at token 0); pieces without it (punctuation, suffixes, byte
    pieces) join the word before. Tokens that spell nothing (special tokens such as a leading <s>,
    the bare U+2581 pieces of padding spaces) belong to the word after them, so the spans tile the
    encoding. Byte-fallback pieces "<0xNN>" are decoded as UTF-8 where they form valid text."""
    special = set(getattr(tokenizer, "added", {}).values())
    pieces = ["" if int(i) in special else p for i, p in zip(ids, tokenizer.pieces(ids))]
    spans: list[list] = []
    for j, p in enumerate(pieces):
        if j == 0 or p.startswith(META):
            spans.append([[], j, j + 1])
        spans[-1][2] = j + 1
        spans[-1][0].append(p)
    # tokens that spell nothing (special tokens, the bare U+2581 pieces of padding spaces) belong to
    # the word after them (the last ones to the word before)
    merged: list[list] = []
    carry = None
    for ps, j0, j1 in spans:
        if carry is not None:
            ps, j0 = carry[0] + ps, carry[1]
            carry = None
        if not "".join(_piece_text(p) for p in ps):
            carry = [ps, j0]
            continue
        merged.append([ps, j0, j1])
    if carry is not None and merged:
        merged[-1][2] = len(pieces)
    out = []
    for ps, j0, j1 in merged:
        buf = bytearray()
        for p in ps:
            if len(p) == 6 and p.startswith("<0x") and p.endswith(">"):
                try:
                    buf.append(int(p[3:5], 16))
                    continue
                except ValueError:
                    pass
            buf += _piece_text(p).encode()
        out.append((buf.decode("utf-8", errors="replace"), j0, j1))
    return out


def word_matrix(A, spans) -> np.ndarray:
    """W[t][w] = sum of A[t][j] over the tokens of word w (float64)."""
    A = np.asarray(A, np.float64)
    if A.ndim != 2:
        raise ValueError(f"expected a frames x tokens matrix, got shape {A.shape}")
    W = np.zeros((A.shape[0], len(spans)), np.float64)
    for w, (_, j0, j1) in enumerate(spans):
        W[:, w] = A[:, j0:j1].sum(axis=1)
    return W


def monotonic_path(W) -> list[int]:
    """c(t), the word of every frame: the path with c(0) = 0 and c(t+1) - c(t) in {0, 1}, its end
    free, that maximises sum_t log(max(W[t][c(t)], 1e-8)) in float64. Ties go to the smaller word
    index: among equal ends the smallest, and a frame whose two predecessors score the same came
    from the smaller one (the path moved on at that frame)."""
    W = np.asarray(W, np.float64)
    T, N = W.shape if W.ndim == 2 else (0, 0)
    if T == 0 or N == 0:
        return []
    L = np.log(np.maximum(W, FLOOR))
    D = np.full((T, N), -np.inf)
    D[0, 0] = L[0, 0]
    for t in range(1, T):
        stay, move = D[t - 1], np.concatenate(([-np.inf], D[t - 1, :-1]))
        D[t] = L[t] + np.maximum(stay, move)
    w = int(np.argmax(D[T - 1]))  # argmax returns the first (smallest) maximiser
    path = [w]
    for t in range(T - 1, 0, -1):
        if w > 0 and D[t - 1, w - 1] >= D[t - 1, w]:
            w -= 1
        path.append(w)
    return path[::-1]


def word_times(path, spans, speed: float = 1.0, eos_frame: int | None = None,
               total_seconds: float | None = None) -> list[dict]:
    """[{"word", "start", "end"}] in seconds of the delivered audio. A word starts at its first
    frame x 0.08 s / speed and ends where the next word starts; the last word ends at the EOS frame
    (eos_frame, where the row stopped by EOS) else at the end of the audio (total_seconds; default:
    the frames' duration); words the path never reached get start = end = the end of the audio.
    Only `speed` scales the times: pitch and volume keep the duration."""
    speed = float(speed or 1.0)
    frame = FRAME_SECONDS / speed
    total = len(path) * frame if total_seconds is None else float(total_seconds)
    first: dict[int, int] = {}
    for t, w in enumerate(path):
        first.setdefault(int(w), t)
    starts = [min(first[w] * frame, total) if w in first else total for w in range(len(spans))]
    out = []
    for w, (word, _, _) in enumerate(spans):
        if w + 1 < len(spans):
            end = starts[w + 1]
        elif eos_frame is not None and w in first:
            end = min(max(eos_frame * frame, starts[w]), total)
        else:
            end = total
        out.append({"word": word, "start": round(starts[w], 6), "end": round(max(end, starts[w]), 6)})
    return out


def diagonality(A) -> float:
    """How well a frames x tokens matrix follows a monotonic path, in [0, 1]: the mean mass on the
    best path over the tokens (monotonic_path with every token a word) times the share of the
    reachable tokens, min(frames, tokens), the path covers. Flat rows over n tokens score about
    1 / n, a row stuck on one token 1 / min(frames, tokens), a sharp diagonal 1."""
    A = np.asarray(A, np.float64)
    if A.ndim != 2 or A.size == 0:
        return 0.0
    path = monotonic_path(A)
    mass = float(np.mean([A[t, c] for t, c in enumerate(path)]))
    cover = (path[-1] + 1) / min(A.shape)
    return float(min(max(mass * cover, 0.0), 1.0))


def timestamps(tokenizer, ids, A, speed: float = 1.0, eos_frame: int | None = None,
               total_seconds: float | None = None) -> list[dict]:
    """word_times of the rows A [frames][len(ids)] of one utterance."""
    spans = word_spans(tokenizer, ids)
    return word_times(monotonic_path(word_matrix(A, spans)), spans, speed, eos_frame, total_seconds)
