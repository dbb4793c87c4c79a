"""numpy float64 restatement of the per-cell confidence definitions (include/classpose_hip.h: cpx_instance_confidence), what
tests/test_cell_confidence_host.py and tests/test_gpu_cell_confidence.py compare against.

For tile t and every label v in 1 .. min(rec_counts[t], max_rec), over the pixels with masks == v:
  votes[t][v-1][c]   pixels whose arg-max class is c (np.argmax: the first maximum wins, a NaN beats every number, the first NaN wins)
  prob_q[t][v-1][c]  sum of q(p_c): m = max_c z_c, e_c = exp(float64(z_c) - m), s = sum_c e_c in class order, p_c = e_c / s,
                     q(p) = rint(p * 2^24) (half to even); a pixel with any non-finite logit adds 0 to every class
  cellprob_q[t][v-1] sum of q(1 / (1 + exp(-float64(z)))); a non-finite z adds 0
One np.bincount per quantity; the sums are exact integers (float64 weights below 2^53).
"""
import numpy as np

Q = float(1 << 24)


def softmax_q(logits: np.ndarray) -> np.ndarray:
    """logits [ncls][n] float32 -> uint64 [ncls][n] quantised softmax, 0 for pixels with a non-finite logit"""
    z = logits.astype(np.float64)
    finite = np.isfinite(z).all(0)
    with np.errstate(all="ignore"):
        m = z.max(0)
        e = np.exp(z - m)
        s = np.zeros_like(m)
        for c in range(z.shape[0]):                    # added in class order
            s = s + e[c]
        q = np.rint((e / s) * Q)
    q[:, ~finite] = 0
    return q.astype(np.uint64)


def sigmoid_q(cellprob: np.ndarray) -> np.ndarray:
    z = cellprob.astype(np.float64)
    with np.errstate(all="ignore"):
        q = np.rint((1.0 / (1.0 + np.exp(-z))) * Q)
    q[~np.isfinite(z)] = 0
    return q.astype(np.uint64)


def instance_confidence(masks, logits, cellprob, rec_counts, max_rec):
    """masks [nT][H][W] uint16, logits [nT][ncls][H][W] float32 or None, cellprob [nT][H][W] float32 or None, rec_counts [nT] ->
    (votes int64 [nT][max_rec][ncls], prob_q uint64 [nT][max_rec][ncls], cellprob_q uint64 [nT][max_rec], valid bool [nT][max_rec]);
    rows where ``valid`` is False are not defined by the entry (here 0)."""
    masks = np.asarray(masks)
    nT = masks.shape[0]
    ncls = 0 if logits is None else logits.shape[1]
    votes = np.zeros((nT, max_rec, ncls), np.int64)
    prob_q = np.zeros((nT, max_rec, ncls), np.uint64)
    cellprob_q = np.zeros((nT, max_rec), np.uint64)
    valid = np.zeros((nT, max_rec), bool)
    for t in range(nT):
        nrec = int(min(max(int(rec_counts[t]), 0), max_rec))
        valid[t, :nrec] = True
        lab = masks[t].reshape(-1).astype(np.int64)
        fg = (lab >= 1) & (lab <= nrec)
        row = lab[fg] - 1
        if logits is not None:
            z = logits[t].reshape(ncls, -1)[:, fg]
            am = np.argmax(z, 0)
            votes[t] = np.bincount(row * ncls + am, minlength=max_rec * ncls).reshape(max_rec, ncls)
            q = softmax_q(z)
            for c in range(ncls):
                prob_q[t, :, c] = np.bincount(row, weights=q[c].astype(np.float64), minlength=max_rec).astype(np.uint64)
        if cellprob is not None:
            q = sigmoid_q(cellprob[t].reshape(-1)[fg])
            cellprob_q[t] = np.bincount(row, weights=q.astype(np.float64), minlength=max_rec).astype(np.uint64)
    return votes, prob_q, cellprob_q, valid
