"""The video detector's tracking tail on the device against the host path it replaces, on the same inputs: a 1024 x 2048 panoptic map
per frame (10 thing + 10 stuff segments, K = 111 entries as a Cityscapes config has), 1 and 32 frames.

  device: ops.track_boxes (semantic filter on, 19-channel logits at stride 8; and filter off) + ops.track_maps — five launches
  host  : what a caller did before: D2H copy of the map, `info` and `bbox`, `KernelIterHead.things_for_tracking` per frame, the two
          maps as the reference's NumPy loops (`map[panoptic_seg == id] = value`), H2D copy of the boxes (no semantic filter: the host
          path never had one)

The tracker and the embedding layers sit between the two halves in both paths and are not timed.  Device times are event times
(`enqueue_host_us`: wall-clock of the calls alone, what the host spends per tail on argument checks, allocation and launches),
host times wall-clock around a synchronised run; warm-up, then the median of `--runs` (>= 20) runs.  The floor beside the device
time is one read of the map plus two writes, 12 bytes per pixel at 6.3 TB/s.

Every measurement is a child process under its own `timeout`; the driver stops at the first one that fails.

    python tools/track_tail_time.py [--runs 20] [--warmup 3] [--out profiles/track_tail_time.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12      # the achievable HBM3E rate the project's other floors use (8 TB/s is the data-sheet peak): not measured by this tool
HO, WO, T, S, MAX_PER_IMG, STRIDE = 1024, 2048, 8, 11, 100, 8
STEP_TIMEOUT_S = {('device', 1): 120, ('device', 32): 180, ('host', 1): 180, ('host', 32): 420}


def _inputs(frames):
    """(seg [B,Ho,Wo], info [B,K,6], nseg [B], bbox [B,K,4], sem [B,19,Ho/8,Wo/8], ids [B,32], n_ids [B]) as NumPy arrays: stuff bands
    as the background, thing rectangles on top; entry order is not segment order."""
    import numpy as np
    K = MAX_PER_IMG + S
    rng = np.random.RandomState(0)
    seg = np.zeros((frames, HO, WO), dtype=np.int32)
    info = np.zeros((frames, K, 6), dtype=np.int32)
    bbox = np.tile(np.asarray([-1, -1, 10, 10], dtype=np.int32), (frames, K, 1))
    for b in range(frames):
        entries = rng.permutation(K)[:20]
        for i in range(20):
            sid, k = i + 1, int(entries[i])
            if i % 2:                                   # stuff band i // 2 of 10
                j = i // 2
                seg[b, j * HO // 10:(j + 1) * HO // 10] = sid
                label = T + j
            else:                                       # a thing rectangle (drawn after the band under it)
                label = i % T
            info[b, k] = (k, label, sid, 0, 0, int(np.float32(0.9 - 0.01 * i).view(np.int32)))
        for i in range(0, 20, 2):
            y0, x0 = rng.randint(0, HO - 200), rng.randint(0, WO - 400)
            seg[b, y0:y0 + rng.randint(40, 200), x0:x0 + rng.randint(40, 400)] = i + 1
        for i in range(20):
            ys, xs = np.nonzero(seg[b] == i + 1)
            k = int(entries[i])
            info[b, k, 3] = info[b, k, 4] = len(ys)
            if len(ys):
                bbox[b, k] = (xs.min(), ys.min(), xs.max(), ys.max())
    nseg = np.full((frames,), 20, dtype=np.int32)
    sem = (rng.randn(frames, T + S, HO // STRIDE, WO // STRIDE) * 3).astype(np.float32)
    ids = np.tile(np.arange(32, dtype=np.int64), (frames, 1))
    ids[:, ::4] = -1
    n_ids = np.full((frames,), 10, dtype=np.int32)
    return seg, info, nseg, bbox, sem, ids, n_ids


def _median_events(fn, warmup, runs):
    import torch
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return round(statistics.median(out), 2), round(min(out), 2)


def _median_wall(fn, warmup, runs):
    import torch
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(out), 2), round(min(out), 2)


def step(kind, frames, warmup, runs):
    """One measurement (child process): prints one JSON line."""
    import numpy as np
    import torch

    import vkn_import
    from importlib import import_module
    vkn = vkn_import.load()
    tt = import_module('video_k_net_amd.track_tail')
    dev = torch.device('cuda:0')
    seg, info, nseg, bbox, sem, ids, n_ids = (torch.from_numpy(a).to(dev) for a in _inputs(frames))
    table = tt.sem_of_label(T, S, False)
    table_d = torch.tensor(table, dtype=torch.int32, device=dev)
    res = dict(kind=kind, frames=frames, runs=runs, warmup=warmup)
    if kind == 'device':
        def tail(filter_on):
            det, labels, rows, segid, count = vkn.ops.track_boxes(seg, info, nseg, T, sem_logits=sem if filter_on else None)
            return vkn.ops.track_maps(seg, segid, count, ids, n_ids, info, table_d)
        res['filter_on_us'], res['filter_on_min_us'] = _median_events(lambda: tail(True), warmup, runs)
        res['filter_off_us'], res['filter_off_min_us'] = _median_events(lambda: tail(False), warmup, runs)
        res['boxes_filter_on_us'], _ = _median_events(lambda: vkn.ops.track_boxes(seg, info, nseg, T, sem_logits=sem), warmup, runs)
        det, labels, rows, segid, count = vkn.ops.track_boxes(seg, info, nseg, T)
        res['maps_us'], _ = _median_events(lambda: vkn.ops.track_maps(seg, segid, count, ids, n_ids, info, table_d), warmup, runs)
        res['floor_us'] = round(frames * HO * WO * 12 / HBM_BYTES_PER_S * 1e6, 2)
        # host cost of ENQUEUEING one tail (no synchronisation inside the timed region): the pointer checks (hipPointerGetAttributes per
        # pointer), output allocation and five launches
        for _ in range(warmup):
            tail(True)
        enq = []
        for _ in range(max(runs, 50)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tail(True)
            enq.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
        res['enqueue_host_us'] = round(statistics.median(enq), 2)
    else:
        KIH = import_module('video_k_net_amd.kernel_iter_head').KernelIterHead
        head_like = type('H', (), dict(num_thing_classes=T))()
        ids_h = ids.cpu().numpy()

        def host():
            seg_h, info_h, bbox_h = seg.cpu().numpy(), info.cpu().numpy(), bbox.cpu().numpy()
            boxes = []
            for b in range(frames):
                acc, labels, bb, scores = KIH.things_for_tracking(head_like, info_h[b], bbox_h[b])
                det = np.zeros((len(acc), 5), dtype=np.float32)
                det[:, :4], det[:, 4] = bb, scores
                boxes.append(torch.from_numpy(det).to(dev))
                track_map, semantic_map = np.zeros(seg_h[b].shape), np.zeros(seg_h[b].shape)
                for i, k in enumerate(acc[:10]):
                    v = ids_h[b, i] + 1
                    track_map[seg_h[b] == info_h[b][k, 2]] = 0 if v == -1 else v
                for k in np.nonzero(info_h[b][:, 2] > 0)[0]:
                    semantic_map[seg_h[b] == info_h[b][k, 2]] = table[info_h[b][k, 1]]
            return boxes
        res['host_us'], res['host_min_us'] = _median_wall(host, min(warmup, 1), runs)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_tail_time.json'))
    ap.add_argument('--step', choices=['device', 'host'], default=None, help='(internal) run one measurement in this process')
    ap.add_argument('--frames', type=int, default=1)
    ap.add_argument('--box', default='', help='free text stored with the result: the machine the numbers come from')
    args = ap.parse_args()
    if args.runs < 20:
        ap.error('--runs must be >= 20')
    if args.step:
        return step(args.step, args.frames, args.warmup, args.runs)
    steps = []
    for frames in (1, 32):
        for kind in ('device', 'host'):
            cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT_S[(kind, frames)]), sys.executable, os.path.abspath(__file__), '--step', kind,
                   '--frames', str(frames), '--runs', str(args.runs), '--warmup', str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:       # a fault, an abort or the time limit: nothing more is started on the GPU
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(f'track_tail_time: step {kind} / {frames} frames ended with status {r.returncode}; stopping')
            steps.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(steps[-1]), flush=True)
    out = dict(tool='track_tail_time', date=time.strftime('%Y-%m-%d'), box=args.box, map=[HO, WO], entries=MAX_PER_IMG + S, segments=20,
               sem_logits=[T + S, HO // STRIDE, WO // STRIDE], floor='12 bytes per pixel (one read of the map, two writes) at 6.3 TB/s (achievable rate assumed, not measured here; peak 8 TB/s)',
               note='the host path has no semantic filter (it never had one) while filter_on_us includes it: host_over_device_* understates the gap',
               steps=steps)
    for frames in (1, 32):
        d = next(s for s in steps if s['kind'] == 'device' and s['frames'] == frames)
        h = next(s for s in steps if s['kind'] == 'host' and s['frames'] == frames)
        out[f'host_over_device_{frames}'] = round(h['host_us'] / d['filter_on_us'], 1)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps({k: v for k, v in out.items() if k != 'steps'}))


if __name__ == '__main__':
    main()
