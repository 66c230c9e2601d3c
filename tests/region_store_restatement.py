"""numpy restatement of the device-resident region store's batch builder (csrc/region_store.hip; include/vilbert_hip_store.h):
gather the spans of the chosen images from the store arrays - the id rule and the clamps of csrc/store_rows.h - into a packed
batch and hand it to THE spec of the packed builder, tests/task_batch_restatement.py. The arithmetic is not stated a second
time. An invalid id owns nothing, not even the mean row: its sample is cleared after the packed restatement has run."""
import numpy as np

import task_batch_restatement as tr


def image_span(store, image_id, total_rows, num_images, max_regions):
    """csrc/store_rows.h: (start, rows, mean, kept) of an id word, (0, 0, 0, 0) for an id outside [0, num_images) - for which no
    store array is indexed."""
    i = int(image_id)
    if not 0 <= i < int(num_images):
        return 0, 0, 0, 0
    mean = store.get("mean_rows")
    return tr.span(store["image_offsets"][i], store["image_offsets"][i + 1], total_rows, None if mean is None else mean[i],
                   max_regions)


def finish_store_batch(store, image_ids, max_regions, ref_box=None, iou_floor=0.0, total_rows=None, num_images=None):
    """store: dict of numpy arrays feat [N, F], boxes [N, 4], image_offsets [I + 1], image_wh [I, 2], mean_rows [I] or None;
    total_rows / num_images: the filled part (default: all of it). Returns what task_batch_restatement.finish_task_batch does."""
    N = store["feat"].shape[0] if total_rows is None else int(total_rows)
    I = len(store["image_offsets"]) - 1 if num_images is None else int(num_images)
    spans = [image_span(store, i, N, I, max_regions) for i in image_ids]
    valid = [kept > 0 for _, _, _, kept in spans]
    rows = [np.arange(start, start + n) for start, n, _, _ in spans]
    take = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
    packed = dict(feat=store["feat"][take], boxes=store["boxes"][take],
                  offsets=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
                  image_wh=np.array([store["image_wh"][int(i)] if ok else (1, 1) for i, ok in zip(image_ids, valid)],
                                    dtype=np.int32).reshape(-1, 2),
                  mean_rows=np.array([mean for _, _, mean, _ in spans], dtype=np.int32))
    out = tr.finish_task_batch(packed, max_regions, ref_box=ref_box, iou_floor=iou_floor)
    for b, ok in enumerate(valid):
        if not ok:
            for o in out:
                o[b] = 0
    return out
