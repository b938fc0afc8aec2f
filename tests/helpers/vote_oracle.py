"""A numpy restatement of the per-pixel vote of the Dropout draws (include/nbc.h, csrc/votes.hpp), written from the definition
alone: the vote word, the winner (torch.argmax's tie rule: the first maximum), the support byte, the invalid word and the ten
statistics per image.  Everything is integer arithmetic; nothing here carries a tolerance."""
import numpy as np

VOTE_STATS = 10


def tally(labels):
    """labels: integer array [D, ...] of the draws' final labels -> uint32 vote words [...]: n1 in bits 0..15, n2 in bits
    16..31.  A label outside {0, 1, 2} votes nowhere."""
    labels = np.asarray(labels)
    n1 = (labels == 1).sum(axis=0).astype(np.uint32)
    n2 = (labels == 2).sum(axis=0).astype(np.uint32)
    assert labels.shape[0] <= 65535
    return n1 | (n2 << np.uint32(16))


def decode(words, draws):
    """-> (label uint8, support uint8, n_win int64, valid bool) of uint32 words under `draws` draws."""
    words = np.asarray(words, dtype=np.uint32).astype(np.int64)
    n1, n2 = words & 0xffff, words >> 16
    valid = n1 + n2 <= draws
    votes = np.stack([draws - n1 - n2, n1, n2])          # class-major: np.argmax takes the first maximum, as torch.argmax does
    label = np.argmax(votes, axis=0)
    n_win = np.max(votes, axis=0)
    support = (255 * n_win) // draws
    label, support, n_win = (np.where(valid, a, 0) for a in (label, support, n_win))
    return label.astype(np.uint8), support.astype(np.uint8), n_win, valid


def stats(words, draws):
    """words uint32 [N, ...] -> int64 [N, 10]: pixels per winning class (0..2), unanimous pixels per class (3..5), the sum of
    n_win (6), invalid words (7), the sums of n1 (8) and n2 (9).  An invalid word is counted in slot 7 alone."""
    words = np.asarray(words, dtype=np.uint32)
    out = np.zeros((words.shape[0], VOTE_STATS), dtype=np.int64)
    for n in range(words.shape[0]):
        w = words[n].reshape(-1)
        label, _, n_win, valid = decode(w, draws)
        wi = w.astype(np.int64)
        for k in range(3):
            won = valid & (label == k)
            out[n, k] = won.sum()
            out[n, 3 + k] = (won & (n_win == draws)).sum()
        out[n, 6] = n_win[valid].sum()
        out[n, 7] = (~valid).sum()
        out[n, 8] = (wi & 0xffff)[valid].sum()
        out[n, 9] = (wi >> 16)[valid].sum()
    return out
