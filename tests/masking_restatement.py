"""A restatement in numpy of the device-side masking of a pre-training batch (include/vilbert_hip_inputs.h, csrc/mask_batch.hip),
built on the hash of tests/dropout_restatement.py. Test infrastructure: tests/test_mask_batch.py checks its statistics on the
CPU, tests/test_mask_batch_gpu.py holds the kernels and the pipeline to it bit for bit. `mask_sample` is written as the per-sample
loops a worker would run (it is also the host side of tools/mask_batch_bench.py); `mask_batch` stacks it.

    u(idx)   = float32(hash(seed, idx) >> 8) * float32(2^-24)      idx = (b * 3 + s) * L + pos,  L = max(T, R)
    s = 0 the token draw, s = 1 the replacement token, s = 2 the region draw
    tokens   eligible 1 .. len - 2 (len = sum(input_mask[b])); selected when u < p; v = u / p in float32:
             v < 0.8 -> mask_token_id, v < 0.9 -> (uint64(hash of stream 1) * vocab_size) >> 32, else unchanged; label = old id
    regions  eligible i < sum(image_mask[b]); selected when u < p: image_label 1 (else -1), zero_row = v < 0.9,
             masked_label[j] = 1 iff some selected i has overlaps[i, j] > float32(0.4)
"""
import numpy as np

from dropout_restatement import vb_hash

RAW_UNMASKED_FIELDS = ("input_ids", "input_mask", "segment_ids", "lm_label_ids", "is_next", "image_feat", "image_loc",
                       "image_target", "image_label", "image_mask", "overlaps")
F08, F09, F04 = np.float32(0.8), np.float32(0.9), np.float32(0.4)
MASK64 = 0xFFFFFFFFFFFFFFFF


def uniform(seed, idx):
    """float32 array in [0, 1): the 24 upper bits of the hash."""
    return (vb_hash(seed, idx) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def site_index(b, stream, L, pos):
    return np.uint64((int(b) * 3 + stream) * int(L)) + np.asarray(pos, dtype=np.uint64)


def batch_seed(seed, i):
    """vilbert.input_pipeline.batch_seed restated: all 64 bits of the splitmix64 finaliser of seed + (i + 1) * 0xD1B54A32D192ED03."""
    z = (int(seed) + (int(i) + 1) * 0xD1B54A32D192ED03) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def mask_sample(b, L, input_ids, input_mask, image_mask, overlaps, seed, vocab_size, mask_token_id, p_select=0.15):
    """One sample, site by site: returns (out_input_ids, lm_label_ids, image_label, masked_label, zero_row)."""
    p = np.float32(p_select)
    T, R = input_ids.shape[0], image_mask.shape[0]
    out_ids, lm = input_ids.astype(np.int64).copy(), np.full(T, -1, dtype=np.int64)
    n_tok = int(input_mask.sum())
    u_tok = uniform(seed, site_index(b, 0, L, np.arange(T)))
    h_rep = vb_hash(seed, site_index(b, 1, L, np.arange(T)))
    for t in range(1, min(n_tok - 1, T)):
        u = u_tok[t]
        if u < p:
            v = u / p
            if v < F08:
                out_ids[t] = mask_token_id
            elif v < F09:
                out_ids[t] = (int(h_rep[t]) * int(vocab_size)) >> 32
            lm[t] = input_ids[t]
    image_label, zero_row = np.full(R, -1, dtype=np.int64), np.zeros(R, dtype=np.uint8)
    masked = np.zeros(R, dtype=bool)
    u_reg = uniform(seed, site_index(b, 2, L, np.arange(R)))
    for i in range(min(int(image_mask.sum()), R)):
        u = u_reg[i]
        if u < p:
            if u / p < F09:
                zero_row[i] = 1
            masked = np.logical_or(masked, overlaps[i] > F04)
            image_label[i] = 1
    return out_ids, lm, image_label, masked.astype(np.int64), zero_row


def mask_arrays(input_ids, input_mask, image_mask, overlaps, seed, vocab_size, mask_token_id, p_select=0.15):
    """The five outputs of vbi_concap_mask_batch for [B, ...] arrays, as a dict."""
    B, T = input_ids.shape
    R = image_mask.shape[1]
    L = max(T, R)
    rows = [mask_sample(b, L, input_ids[b], input_mask[b], image_mask[b], overlaps[b], seed, vocab_size, mask_token_id, p_select)
            for b in range(B)]
    names = ("input_ids", "lm_label_ids", "image_label", "masked_label", "zero_row")
    dtypes = (np.int64, np.int64, np.int64, np.int64, np.uint8)
    shapes = ((B, T), (B, T), (B, R), (B, R), (B, R))
    return {n: np.array([r[k] for r in rows], dtype=d).reshape(s) for k, (n, d, s) in enumerate(zip(names, dtypes, shapes))}


def mask_batch(raw, seed, vocab_size, mask_token_id, p_select=0.15):
    """vilbert.input_pipeline.mask_batch restated: the unmasked raw dict (RAW_UNMASKED_FIELDS) -> the raw dict finish_batch
    takes (new arrays; `raw` is left as it is)."""
    m = mask_arrays(raw["input_ids"], raw["input_mask"], raw["image_mask"], raw["overlaps"], seed, vocab_size, mask_token_id,
                    p_select)
    out = {n: raw[n] for n in RAW_UNMASKED_FIELDS if n != "overlaps"}
    feat = raw["image_feat"].copy()
    feat[m["zero_row"] != 0] = 0
    out.update(input_ids=m["input_ids"], lm_label_ids=m["lm_label_ids"], image_label=m["image_label"], image_feat=feat,
               masked_label=m["masked_label"])
    return out


def make_unmasked_batch(batch, tokens=36, regions=36, feat_dim=2048, n_classes=1601, vocab=30522, seed=0, n_tok=None, n_box=None):
    """An unmasked worker batch with the loader's conventions: [CLS] ids [SEP] and zero padding, ragged numbers of boxes, padded
    regions zero, overlaps = a symmetric matrix with a unit diagonal on the real boxes, zero-padded, with a few entries placed
    EXACTLY at float32(0.4) (which must not mask) and just above it. n_tok / n_box: per-sample lengths, drawn when None."""
    g = np.random.RandomState(seed)
    n_tok = g.randint(min(3, tokens), tokens + 1, size=batch) if n_tok is None else np.asarray(n_tok)
    n_box = g.randint(1, regions + 1, size=batch) if n_box is None else np.asarray(n_box)
    tok_ok = np.arange(tokens)[None, :] < n_tok[:, None]
    box_ok = np.arange(regions)[None, :] < n_box[:, None]
    ids = g.randint(1000 % vocab, vocab, size=(batch, tokens)).astype(np.int64) * tok_ok
    ids[:, 0] = np.where(n_tok > 0, 101 % vocab, 0)
    for b in range(batch):
        if n_tok[b] > 1:
            ids[b, n_tok[b] - 1] = 102 % vocab
    feat = (g.rand(batch, regions, feat_dim).astype(np.float32) + np.float32(0.5)) * box_ok[:, :, None]
    loc = g.rand(batch, regions, 5).astype(np.float32) * box_ok[:, :, None]
    ov = g.rand(batch, regions, regions).astype(np.float32)
    ov = np.minimum(ov, ov.transpose(0, 2, 1))
    pick = g.rand(batch, regions, regions)
    ov[pick < 0.10] = F04                                   # exactly the threshold: not above it
    ov[(pick >= 0.10) & (pick < 0.15)] = np.nextafter(F04, np.float32(1))
    eye = np.eye(regions, dtype=bool)[None]
    ov = np.where(eye, np.float32(1), ov) * (box_ok[:, :, None] & box_ok[:, None, :])
    target = g.rand(batch, regions, n_classes).astype(np.float32)
    target /= target.sum(-1, keepdims=True)
    return dict(input_ids=ids, input_mask=tok_ok.astype(np.int64), segment_ids=np.zeros((batch, tokens), np.int64),
                lm_label_ids=np.full((batch, tokens), -1, np.int64), is_next=g.randint(0, 2, size=batch).astype(np.int64),
                image_feat=feat, image_loc=loc, image_target=target, image_label=np.full((batch, regions), -1, np.int64),
                image_mask=box_ok.astype(np.int64), overlaps=ov.astype(np.float32))
