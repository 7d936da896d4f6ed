"""float64 numpy restatement of the vocabulary cross-entropy kernels (csrc/lm_loss.hip, include/mmfd.h
mmfd_vocab_xent_fwd / mmfd_vocab_xent_bwd): what tests/test_lm_loss_cpu.py holds against torch's
cross_entropy and its autograd, and what tests/test_lm_loss_gpu.py holds the kernels against."""
import numpy as np

IGNORE = -100


def xent_fwd(logits, labels, eps=0.0, rows_per_seq=None):
    """logits [R, V], labels int64 [R] (IGNORE = not scored): dict of
    loss_rows [R] = lse - (1 - eps) z[y] - (eps / V) sum_v z[v] (0 where ignored), lse [R], mean (over the valid
    rows; NaN without one), n_valid, seq_sums [R / rows_per_seq] (or None)"""
    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    R, V = z.shape
    m = z.max(axis=1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
    valid = y != IGNORE
    zy = z[np.arange(R), np.where(valid, y, 0)]
    loss = lse - (1.0 - eps) * zy
    if eps != 0.0:
        loss = loss - (eps / V) * z.sum(axis=1)
    loss = np.where(valid, loss, 0.0)
    n = int(valid.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.float64(loss.sum()) / np.float64(n)
    seq = loss.reshape(-1, rows_per_seq).sum(axis=1) if rows_per_seq else None
    return dict(loss_rows=loss, lse=lse, mean=mean, n_valid=n, seq_sums=seq)


def xent_bwd(logits, labels, lse, eps=0.0, upstream=None, n_valid=None, rows_per_seq=None):
    """dlogits [R, V] = g_r (exp(z - lse_r) - (1 - eps) [v == y_r] - eps / V); g_r = 0 for an ignored row, else
    upstream / n_valid in the mean form (n_valid given; upstream a scalar, None = 1) or upstream[r // rows_per_seq]"""
    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    R, V = z.shape
    valid = y != IGNORE
    if n_valid is not None:
        with np.errstate(invalid="ignore", divide="ignore"):
            g = np.full(R, (1.0 if upstream is None else float(upstream)) / np.float64(n_valid))
    else:
        g = np.repeat(np.asarray(upstream, dtype=np.float64), rows_per_seq)
    g = np.where(valid, g, 0.0)
    d = np.exp(z - np.asarray(lse, dtype=np.float64)[:, None]) - eps / V
    d[np.arange(R)[valid], y[valid]] -= 1.0 - eps
    d = g[:, None] * d
    d[~valid] = 0.0
    return d
