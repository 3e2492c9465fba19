#!/usr/bin/env python
"""Rate of the overlay stage, maps + images -> faded patches: 1000 rows over 200 images of 512 x 512 (5 boxes of 64 x 64 per image),
sigma 10, the whole-image variant (`Cluster.load_and_apply_alpha_bbox`); normalised maps and uint8 images already on the device.

  filter    overlay.gaussian_filter(maps, 10, 'clamp'): one dm_gaussian_filter_maps for the 200 maps
  blend     dm_overlay_blend for the 1000 rows on the filtered maps: overlay.overlay_rows(...) minus the filter, and the whole call
  scipy     the reference's own lines on the same inputs in the same run, on this machine's CPU, for scale: per image
            `gaussian_filter(alpha, sigma=10)`, `T*(T>0)`, and per ROW the reference's float64 blend of the WHOLE image followed by
            the crop (it blends the image once per patch, cluster.py:93-110) - on --scipy-images images, reported per image and row

Every time is HOST clock (perf_counter around work that ends with a device synchronisation), warm-up first, median of --reps.  No
threshold hangs on these numbers.

    python tools/overlay_rate.py [--images 200] [--rows-per-image 5] [--reps 10] [--scipy-images 20] [--out profiles/overlay_rate.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--rows-per-image", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scipy-images", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_rate.txt"))
    a = ap.parse_args()
    import torch
    from diff_mining_amd import overlay as O
    if not torch.cuda.is_available():
        sys.exit("overlay_rate needs the GPU: a rate is measured there or not at all")
    dev = torch.device("cuda", 0)
    H = W = 512
    k, sigma = 64, 10
    rng = np.random.default_rng(20261021)
    maps_h = [rng.random((H, W)).astype(np.float32) for _ in range(a.images)]
    images_h = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(a.images)]
    image = np.repeat(np.arange(a.images), a.rows_per_image)
    x0, y0 = rng.integers(0, H - k + 1, image.size), rng.integers(0, W - k + 1, image.size)
    rows = {"image": image, "x_start": x0, "y_start": y0, "x_end": x0 + k, "y_end": y0 + k}
    maps = [torch.from_numpy(m).to(dev) for m in maps_h]
    images = [torch.from_numpy(i).to(dev) for i in images_h]

    def clock(fn):
        for _ in range(2):
            fn()
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)
    t_filter = clock(lambda: O.gaussian_filter(maps, sigma, "clamp"))
    t_all = clock(lambda: O.overlay_rows(images, maps, rows, "image", sigma))
    got = O.overlay_rows(images, maps, rows, "image", sigma)

    from scipy.ndimage import gaussian_filter
    n = min(a.scipy_images, a.images)
    tf, tb, same = [], [], True
    for b in range(n):
        t0 = time.perf_counter()
        T = gaussian_filter(maps_h[b], sigma=sigma)
        T = T * (T > 0)
        tf.append((time.perf_counter() - t0) * 1e3)
        I = images_h[b] / 255.0
        for q in np.flatnonzero(image == b):
            t0 = time.perf_counter()
            T3 = np.stack((T, T, T), axis=-1)
            A = np.zeros_like(I)
            A[:T3.shape[0], :T3.shape[1], :] = T3
            R = 0.05 * I + 0.95 * (A * I + (1 - A))
            R = R[x0[q]:x0[q] + k, y0[q]:y0[q] + k]
            u8 = (R * 255).astype(np.uint8)
            tb.append((time.perf_counter() - t0) * 1e3)
            same = same and np.array_equal(u8, got["blended"][q].cpu().numpy())
    n_rows = image.size
    blend = t_all[0] - t_filter[0]
    lines = [
        f"overlay rate: {n_rows} rows of {k}x{k} over {a.images} images of {H}x{W}, sigma {sigma}, variant 'image'; maps and images on the device",
        f"device: {torch.cuda.get_device_name(0)}; every time is HOST clock around work that ends with a synchronisation, median of {a.reps}",
        f"filter (dm_gaussian_filter_maps, {a.images} maps, with the upload of its tables): {t_filter[0]:.3f} ms (min {t_filter[1]:.3f}, max {t_filter[2]:.3f}) "
        f"= {a.images / t_filter[0] * 1e3:.0f} maps/s",
        f"filter + blend (overlay.overlay_rows, one filter call and one dm_overlay_blend, with packing the images and the tables): {t_all[0]:.3f} ms "
        f"(min {t_all[1]:.3f}, max {t_all[2]:.3f}) = {n_rows / t_all[0] * 1e3:.0f} rows/s",
        f"blend and packing, by difference: {blend:.3f} ms",
        f"scipy + numpy, the reference's lines on this machine's CPU ({n} images, {len(tb)} rows): gaussian_filter + clamp median {statistics.median(tf):.2f} ms "
        f"per image; whole-image float64 blend + crop median {statistics.median(tb):.2f} ms per row; scaled to the full table "
        f"{statistics.median(tf) * a.images + statistics.median(tb) * n_rows:.0f} ms; bytes equal to the device's on those rows: {same}",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
