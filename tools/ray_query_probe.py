#!/usr/bin/env python3
"""Ray-query timings on one GPU (DESIGN.md s5 "Ray queries"): K3 (bunny + ground) at 1920 x 1080, the frame's
2,073,600 primary rays handed to srt_trace_rays_device in three orders -- (a) the renderer's tile order (8 x 8 pixels a wave), (b)
row-major, (c) randomly permuted -- beside ms_primary of the reference-frame render with the wave-triangle-queue variant (flags 2 << 8:
the same per-lane walk, specialised to rays from the origin) and of the shipped pipeline; the occlusion query on the frame's shadow rays;
the host entry point end to end for 1 ray and for all of them.
--shade: instead, the shaded-ray query on the same frame's rays at 1 and 16 light samples, in row-major order and shuffled: (a)
srt_shade_rays_device, (b) the camera-mode srt_render_device of the same frame (identity matrix: the same rays, the same result), (c) the
composition of the older queries -- srt_trace_rays_device, shadow rays built with torch, srt_occluded_device on hits x samples rays (it
stops short of shading: no Phong, no tone map).
--range: instead, what the per-ray t interval costs (srt_trace_rays_range_device, srt_occluded_range_device) on the same frame's rays,
row-major and shuffled: the unbounded closest-hit call beside the range call with (0, +inf) -- the same answers -- and with t_max at the
frame's median hit t; both forms of occlusion on the frame's shadow rays.  Every figure is the median of --rounds rounds of --reps
calls, the forms alternating within a round, with the rounds' minimum and maximum: the spread the ratios are to be read against.
--multi: instead, the K nearest hits in one walk (srt_trace_rays_multi_device) on the same frame's rays in the three orders: k = 1, 4, 8
and 16 without an interval beside srt_trace_rays_range_device with (0, +inf) on the same rays in the same rounds; k hits by the next_up
chain of k range calls (t_min made on the device with torch.nextafter) beside the one multi call; the host forms end to end at k = 4.
--shade-range: instead, what the interval costs the shaded query (srt_shade_rays_range_device) on the same frame's rays, row-major and
shuffled, at 1 and 16 light samples: the unbounded srt_shade_rays_device beside the range call with (0, +inf) -- the same bytes -- and
with t_min just behind the frame's hit (next_up(t): the colour at the exit point / behind the first surface), in the same rounds.
--surface: instead, the surface at a hit (srt_surface_rays_device, srt_surface_hits_device) on the same frame's rays, row-major and
shuffled, in the same rounds: srt_trace_rays_device (the yardstick: k_query_closest on the same rays), srt_surface_rays_device with all
outputs and with normal + bounce only, srt_surface_hits_device on the frame's hits, and srt_surface_rays_device of the OTHER store form
-- the library built with -DSRT_SURFACE_LANE_STORES (python -m simple_raytracer_amd.build --surface-lane-stores), loaded beside the
shipped one, on a scene of its own.
--paths: instead, mirror paths of the same frame at depth 1 / 3 and 1 / 16 light samples, four ways in one run: the chain of existing device
calls, srt_shade_paths_device on rays built beforehand, srt_render_paths_device, and at depth 1 srt_render_device.
--shadow-rule: instead, what a shadow rule costs the two path calls on the same frame at depth 1 / 3 and 1 / 16 light samples, in one run:
srt_shade_paths_device and srt_render_paths_device with no rule (the existing kernels) beside (1e-3, 1, 0) and (1e-3, 1, SELF).
--masked: instead, what the visibility masks cost on the same frame, in one run: srt_trace_rays_range_device with (0, +inf) -- the existing
kernel, the yardstick -- beside srt_trace_rays_masked_device with every mask all ones (the same answers) and with the bunny hidden by the
ray masks; and srt_shade_paths_shadow_device under (1e-3, 1, 0) beside srt_shade_paths_masked_device with all ones and with the bunny hidden
from every ray kind, at depth 3 and 1 / 16 light samples.
--refract: instead, what the REFRACT build costs the path calls on the rays of the same frame at depth 3 and 1 / 16 light samples, in one
run: srt_shade_paths_masked_device under (1e-3, 1, 0) with all-ones masks -- the existing kernel, the yardstick -- beside
srt_shade_paths_refract_device with an all-zero table (the same walks to the bit: the price of the build alone) and with the bunny as glass of
index 1.5 (other walks: for information).  Beside every ratio stands the yardstick's own round-to-round spread.
--fresnel: instead, what the Fresnel split costs the path calls on the rays of the same frame at depth 3 and 1 / 16 light samples, with the
bunny as glass of index 1.5, in one run: srt_shade_paths_refract_device -- the yardstick -- beside srt_shade_paths_fresnel_device with an
all-negative f0 (nothing splits, the same bits: the price of the build alone) and with f0 = 0.04 (the price of the side walks), and beside the
chain of device calls that computes the same pixels.
--ao: instead, ambient occlusion on the rays of the same frame at 16 and 64 cosine directions, t in (1e-3, 60), in one run: the chain the
fused calls replace -- srt_surface_rays_device, the torch operations that build the frame and the n x K x 6 rays (a caller's own kernel
would be one launch; torch takes a dozen elementwise ones), srt_occluded_masked_device with a ray mask of 0 on the rays of a miss, a torch
reduction: the yardstick -- beside srt_ao_rays_device and srt_ao_hits_device (on a render's hits) under the shipped rule for the deal of rays
to waves and under either deal alone (the libraries of python -m simple_raytracer_amd.build --ao-deals, loaded beside the shipped one).
--render-ao: instead, ambient occlusion over the same frame's own pixels at 16 and 64 cosine directions, t in (1e-3, 60), in one run: the
shipped calls on rays torch makes per call (24 B a pixel, four elementwise launches) -- srt_ao_rays_device and, on a render's hits,
srt_ao_hits_device: the yardsticks -- beside srt_render_ao_device and srt_render_ao_hits_device without a table, with a 4 x 4 table of
rotations, and with that table and the bent normal.
--points: instead, the closest-point query (srt_closest_points_device) on the hit points of the same frame, pushed off the surface towards
the camera by a few offsets, over a few radii on a sub-sample of the hits and with no radius (+inf: every triangle is a candidate) on a
smaller one, in one run beside srt_trace_rays_device on the rays of the same pixels -- the yardstick of what a walk costs -- and the node and
triangle tests per point from the counting build.
--nearest: the table of --points with srt_nearest_points_device (the bound shrinks) beside srt_closest_points_device, the yardstick, on the same
points in the same rounds at every radius; the outputs of the two are compared on the way.
--signed: srt_signed_points_device (the default table's 3 directions, parity) on the points of --nearest without a radius, beside the chain it
replaces on the calls that existed before it, in the same rounds: srt_nearest_points_device, torch writing the n x 3 rays,
srt_trace_rays_multi_device for n_hits alone, the vote and the sign in torch.  Equal bits are asserted.  Also srt_nearest_points_device
alone (what the sign costs on top of it) and containment only (no nearest phase).
--points-multi: the K nearest triangles per point (srt_closest_points_multi_device, srt_nearest_points_multi_device; k = 1, 4, 16) on the
points of --nearest at radii 1, 4, 16 and none, beside srt_closest_points_device and srt_nearest_points_device in the same rounds; equal bits
of column 0 and of the two forms are asserted, the counters printed.
--segments: instead, the segment query (srt_closest_segments_device) on every 64th and on every 4th hit point of the same frame: point segments beside
srt_closest_points_device (the price of the policy), segments of length 4 and 32 in random directions at radius 1 and 4 beside the point call
at the midpoint with radius r + L / 2 (what a caller could do before), and the same through the build without box test 2 when it is there.
Usage: python tools/ray_query_probe.py [--reps N] [--trace] [--segments | --shade | --range | --shade-range | --multi | --surface | --paths | --shadow-rule | --masked | --refract | --fresnel | --ao | --render-ao | --points | --nearest | --signed | --points-multi [--rounds R]]     (--trace: few repetitions, for a run under rocprofv3 --kernel-trace --stats)"""
import argparse, os, sys, time
import numpy as np
import torch                                   # first: torch initialises HIP before the library does

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402

W, H, FOCAL = 1920, 1080, 400.0


def frame_rays():
    """The reference frame's rays: origin 0, direction (i, j, focal), row-major."""
    i0, j0 = int(-np.float32(W) / 2), int(-np.float32(H) / 2)
    r = np.zeros((H, W, 6), np.float32)
    r[..., 3] = (i0 + np.arange(W)).astype(np.float32)[None, :]
    r[..., 4] = (j0 + np.arange(H)).astype(np.float32)[:, None]
    r[..., 5] = FOCAL
    return r.reshape(-1, 6)


def tile_order():
    """Pixel indices in the order the render kernels deal them: 16 x 16 pixels a workgroup, 8 x 8 a wave, row-major inside."""
    y, x = np.mgrid[0:H, 0:W]
    key = ((y // 16) * ((W + 15) // 16) + x // 16) * 256 + (((y % 16) // 8) * 2 + (x % 16) // 8) * 64 + (y % 8) * 8 + x % 8
    return np.argsort(key.reshape(-1), kind="stable")


def timed(fn, reps, stream):
    """ms a call: events on `stream`, the stream the calls are enqueued on (a stream of its own: NULL would be the scene's own stream)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(); fn(); stream.synchronize()
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream); stream.synchronize()
    return a.elapsed_time(b) / reps


def rounds_of(forms, reps, rounds, stream):
    """forms: name -> call.  Per form the ms a call of every round (the forms alternate within a round)."""
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            ms[k].append(timed(fn, reps, stream))
    return ms


def report(title, ms, yard=None):
    """One line per form: median, minimum and maximum of its rounds, and the median over the median of form `yard` (default: the first)."""
    med = {k: float(np.median(v)) for k, v in ms.items()}
    yard = next(iter(med)) if yard is None else yard
    for k, v in ms.items():
        print(f"{title:34s} {k:34s} {med[k]:8.3f} {min(v):8.3f} {max(v):8.3f} {med[k] / med[yard]:7.3f}")


def shade_section(reps):
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    rays = frame_rays()
    n = rays.shape[0]
    eye = np.eye(4, dtype=np.float32).reshape(-1)
    tri_obj = torch.from_numpy(g.flat.tri_obj.astype(np.int64)).to(dev)
    hit = torch.empty(n, dtype=torch.int32, device=dev); t = torch.empty(n, dtype=torch.float32, device=dev)
    lin = torch.empty((n, 3), dtype=torch.float32, device=dev); rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    f8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    print(f"shaded rays, K3 ground_bunny {W}x{H}: {n} rays, {reps} repetitions each; ms a call")
    print(f"{'samples':>7s} {'order':>9s} {'(a) shade_rays':>15s} {'(b) render':>11s} {'(c) trace+occluded':>19s} {'(a)/(b)':>8s} {'(a)/(c)':>8s}   same rgb8 as the frame")
    for L in (1, 16):
        lights = abi.light_staircase(g.light, L)
        p_frame = abi.make_params(W, H, lights, focal=FOCAL, ray_matrix=eye, flags=abi.SRT_FLAG_NO_TIMING)
        p_rays = abi.make_params(1, 1, lights)
        d_lights = torch.from_numpy(lights).to(dev)
        mb = timed(lambda: ds.render_device(p_frame, stream=cur, rgb8=f8.data_ptr()), reps, side)
        frame8 = f8.cpu().numpy().reshape(-1, 3)
        for name, order in (("row-major", np.arange(n)), ("shuffled", np.random.default_rng(1).permutation(n))):
            d_rays = torch.from_numpy(np.ascontiguousarray(rays[order])).to(dev)
            torch.cuda.synchronize()
            ma = timed(lambda: ds.shade_rays_device(n, d_rays.data_ptr(), p_rays, stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr(), rgb_linear=lin.data_ptr(),
                                                    rgb8=rgb8.data_ptr()), reps, side)
            ok = np.array_equal(rgb8.cpu().numpy(), frame8[order])

            def composed():
                ds.trace_rays_device(n, d_rays.data_ptr(), stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr())
                with torch.cuda.stream(side):
                    sel = torch.nonzero(hit >= 0).squeeze(1)
                    r = d_rays[sel]
                    so = r[:, 0:3] + r[:, 3:6] * t[sel, None]
                    sray = torch.cat([so[:, None, :].expand(-1, L, -1), d_lights[None, :, :] - so[:, None, :]], dim=2).reshape(-1, 6).contiguous()
                    skip = tri_obj[hit[sel].long()].to(torch.int32)[:, None].expand(-1, L).reshape(-1).contiguous()
                    occ = torch.empty(sray.shape[0], dtype=torch.uint8, device=dev)
                ds.occluded_device(sray.shape[0], sray.data_ptr(), occ.data_ptr(), skip_obj=skip.data_ptr(), stream=cur)
                return occ
            mc = timed(composed, reps, side)
            print(f"{L:7d} {name:>9s} {ma:15.3f} {mb:11.3f} {mc:19.3f} {ma / mb:8.2f} {ma / mc:8.2f}   {ok}")
            assert ok


def range_section(reps, rounds):
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    rays = frame_rays()
    n = rays.shape[0]
    frame = ds.render(g.params(W, H, 1), want=("hit_id", "t"))
    hit_ref, t_ref = frame["hit_id"].reshape(-1), frame["t"].reshape(-1)
    sel = hit_ref >= 0
    t_med = np.float32(np.median(t_ref[sel]))
    hit = torch.empty(n, dtype=torch.int32, device=dev); t = torch.empty(n, dtype=torch.float32, device=dev)

    print(f"t interval, K3 ground_bunny {W}x{H}: {n} rays, {int(sel.sum())} hits, median hit t {t_med:.6g}; {rounds} rounds of {reps} calls, forms alternating; ms a call")
    print(f"{'rays':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ first':>7s}")
    for name, order in (("closest hit, row-major", np.arange(n)), ("closest hit, shuffled", np.random.default_rng(1).permutation(n))):
        d_rays = torch.from_numpy(np.ascontiguousarray(rays[order])).to(dev)
        d_open = torch.from_numpy(np.tile(np.float32([0.0, np.inf]), (n, 1))).to(dev)
        d_far = torch.from_numpy(np.tile(np.array([0.0, t_med], np.float32), (n, 1))).to(dev)
        torch.cuda.synchronize()
        call = lambda tr: (lambda: ds.trace_rays_device(n, d_rays.data_ptr(), stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr(), t_range=tr))
        ms = rounds_of({"unbounded": call(None), "range (0, +inf)": call(d_open.data_ptr()), "range (0, median hit t)": call(d_far.data_ptr())}, reps, rounds, side)
        report(name, ms, "unbounded")
        # what the forms answer: (0, +inf) the frame, (0, median) the frame's hits up to the median and misses beyond
        call(d_open.data_ptr())(); side.synchronize()
        assert np.array_equal(hit.cpu().numpy(), hit_ref[order]) and np.array_equal(t.cpu().numpy().view(np.uint32), t_ref[order].view(np.uint32))
        call(d_far.data_ptr())(); side.synchronize()
        near = sel[order] & (t_ref[order] <= t_med)
        assert np.array_equal(hit.cpu().numpy(), np.where(near, hit_ref[order], -1))
    # occlusion: the frame's shadow rays as segments (so = d * t, sd = L - so, range (0, 1)), the hit object skipped
    L = np.asarray(g.light, np.float32).reshape(1, 3)
    so = rays[sel, 3:6] * t_ref[sel, None]
    sray = np.ascontiguousarray(np.concatenate([so, L - so], 1), np.float32)
    skip = g.flat.tri_obj[hit_ref[sel]].astype(np.int32)
    m = sray.shape[0]
    occ = torch.empty(m, dtype=torch.uint8, device=dev)
    for name, order in (("occlusion, frame order", np.arange(m)), ("occlusion, shuffled", np.random.default_rng(2).permutation(m))):
        d_s = torch.from_numpy(np.ascontiguousarray(sray[order])).to(dev); d_k = torch.from_numpy(np.ascontiguousarray(skip[order])).to(dev)
        d_open = torch.from_numpy(np.tile(np.float32([0.0, np.inf]), (m, 1))).to(dev)
        d_seg = torch.from_numpy(np.tile(np.float32([0.0, 1.0]), (m, 1))).to(dev)
        torch.cuda.synchronize()
        call = lambda tr: (lambda: ds.occluded_device(m, d_s.data_ptr(), occ.data_ptr(), skip_obj=d_k.data_ptr(), stream=cur, t_range=tr))
        ms = rounds_of({"unbounded": call(None), "range (0, +inf)": call(d_open.data_ptr()), "range (0, 1): segments": call(d_seg.data_ptr())}, reps, rounds, side)
        report(name, ms, "unbounded")
        counts = []
        for tr in (None, d_open.data_ptr(), d_seg.data_ptr()):
            call(tr)(); side.synchronize()
            counts.append(int(occ.sum().item()))
        print(f"{'':34s} occluded of {m}: unbounded {counts[0]}, (0, +inf) {counts[1]}, (0, 1) {counts[2]}")
        assert counts[0] == counts[1] >= counts[2]


def shade_range_section(reps, rounds):
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    rays = frame_rays()
    n = rays.shape[0]
    frame = ds.render(g.params(W, H, 1), want=("hit_id", "t"))
    hit_ref, t_ref = frame["hit_id"].reshape(-1), frame["t"].reshape(-1)
    behind = np.stack([np.nextafter(t_ref, np.float32(np.inf)), np.full(n, np.inf, np.float32)], axis=1).astype(np.float32)      # a miss: (inf, inf)
    hit = torch.empty(n, dtype=torch.int32, device=dev); t = torch.empty(n, dtype=torch.float32, device=dev)
    lin = torch.empty((n, 3), dtype=torch.float32, device=dev); rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=dev)
    print(f"shaded rays with a t interval, K3 ground_bunny {W}x{H}: {n} rays, {int((hit_ref >= 0).sum())} hits; {rounds} rounds of {reps} calls, forms alternating; ms a call")
    print(f"{'samples, rays':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ first':>7s}")
    for L in (1, 16):
        p = abi.make_params(1, 1, abi.light_staircase(g.light, L))
        for name, order in (("row-major", np.arange(n)), ("shuffled", np.random.default_rng(1).permutation(n))):
            d_rays = torch.from_numpy(np.ascontiguousarray(rays[order])).to(dev)
            d_open = torch.from_numpy(np.tile(np.float32([0.0, np.inf]), (n, 1))).to(dev)
            d_behind = torch.from_numpy(np.ascontiguousarray(behind[order])).to(dev)
            torch.cuda.synchronize()
            call = lambda tr: (lambda: ds.shade_rays_device(n, d_rays.data_ptr(), p, stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr(), rgb_linear=lin.data_ptr(),
                                                            rgb8=rgb8.data_ptr(), t_range=tr))
            forms = {"unbounded": call(None), "range (0, +inf)": call(d_open.data_ptr()), "range (next_up(t), +inf)": call(d_behind.data_ptr())}
            report(f"{L:2d} samples, {name}", rounds_of(forms, reps, rounds, side))
            # what the forms answer: (0, +inf) the unbounded call's bytes; behind the first hit another triangle or nothing
            got = []
            for tr in (None, d_open.data_ptr(), d_behind.data_ptr()):
                call(tr)(); side.synchronize()
                got.append((hit.cpu().numpy(), t.cpu().numpy().view(np.uint32), lin.cpu().numpy().view(np.uint32), rgb8.cpu().numpy()))
            assert np.array_equal(got[0][0], hit_ref[order]) and all(np.array_equal(a, b) for a, b in zip(got[0], got[1]))
            second = got[2][0]
            assert ((second < 0) | (second != got[0][0])).all()
            print(f"{'':34s} hits: unbounded {int((got[0][0] >= 0).sum())}, behind the first hit {int((second >= 0).sum())}")


def multi_section(reps, rounds):
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    rays = frame_rays()
    n = rays.shape[0]
    KS = (1, 4, 8, 16)
    hit = torch.empty(n, dtype=torch.int32, device=dev); t = torch.empty(n, dtype=torch.float32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    mhit = torch.empty(n * 16, dtype=torch.int32, device=dev); mt = torch.empty(n * 16, dtype=torch.float32, device=dev)
    d_open = torch.from_numpy(np.tile(np.float32([0.0, np.inf]), (n, 1))).to(dev)
    d_tr = d_open.clone()
    inf = torch.full((n,), float("inf"), device=dev)
    print(f"K nearest hits, K3 ground_bunny {W}x{H}: {n} rays; {rounds} rounds of {reps} calls, forms alternating; ms a call (n_hits, hit_id, t written)")
    print(f"{'rays':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ first':>7s}")

    for name, order in (("(a) tile order", tile_order()), ("(b) row-major", np.arange(n)), ("(c) randomly permuted", np.random.default_rng(1).permutation(n))):
        d_rays = torch.from_numpy(np.ascontiguousarray(rays[order])).to(dev)
        torch.cuda.synchronize()
        rng_call = lambda: ds.trace_rays_device(n, d_rays.data_ptr(), stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr(), t_range=d_open.data_ptr())
        multi = lambda k: (lambda: ds.trace_rays_multi_device(n, d_rays.data_ptr(), k, stream=cur, n_hits=cnt.data_ptr(), hit_id=mhit.data_ptr(), t=mt.data_ptr()))
        forms = {"range (0, +inf)": rng_call}
        forms.update({f"multi k = {k}": multi(k) for k in KS})
        report(name, rounds_of(forms, reps, rounds, side))
        # column 0 of the multi call is the range call
        rng_call(); multi(8)(); side.synchronize()
        assert torch.equal(mhit[:n * 8].view(n, 8)[:, 0], hit) and torch.equal(mt[:n * 8].view(n, 8)[:, 0].view(torch.int32), t.view(torch.int32))
        hist = torch.bincount(cnt.clamp(max=17).long(), minlength=18).cpu().numpy()
        print(f"{'':34s} hits per ray (0, 1, 2, ...; last = 17 and more): {hist.tolist()}")
        if name != "(b) row-major":
            continue

        def chain(k):
            def run():
                with torch.cuda.stream(side):
                    d_tr.copy_(d_open)
                for j in range(k):
                    ds.trace_rays_device(n, d_rays.data_ptr(), stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr(), t_range=d_tr.data_ptr())
                    if j + 1 < k:
                        with torch.cuda.stream(side):
                            d_tr[:, 0] = torch.where(hit >= 0, torch.nextafter(t, inf), inf)
            return run
        for k in (4, 8):
            report(f"{k} hits, row-major", rounds_of({f"multi k = {k}, one call": multi(k), f"next_up chain, {k} range calls": chain(k)}, reps, rounds, side))
    # the host forms, end to end (staging, wait, copies back)
    r = np.ascontiguousarray(rays)
    tr = np.tile(np.float32([0.0, np.inf]), (n, 1))
    ms = {"srt_trace_rays_range (hit_id, t)": [], "srt_trace_rays_multi k = 4 (n_hits, hit_id, t)": []}
    for _ in range(rounds):
        for key, fn in (("srt_trace_rays_range (hit_id, t)", lambda: ds.trace_rays(r, want=("hit_id", "t"), t_range=tr)),
                        ("srt_trace_rays_multi k = 4 (n_hits, hit_id, t)", lambda: ds.trace_rays_multi(r, 4, want=("n_hits", "hit_id", "t")))):
            fn()
            t0 = time.perf_counter()
            for _ in range(3):
                fn()
            ms[key].append((time.perf_counter() - t0) / 3 * 1e3)
    for key, v in ms.items():
        print(f"{'host form, end to end':34s} {key:46s} {float(np.median(v)):8.3f} {min(v):8.3f} {max(v):8.3f}")


def surface_section(reps, rounds):
    from simple_raytracer_amd import build
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    lane = lib.DeviceScene(g.flat, library=lib.load(build.build_surface_lane_stores()))
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    rays = frame_rays()
    n = rays.shape[0]
    hit = torch.empty(n, dtype=torch.int32, device=dev); t = torch.empty(n, dtype=torch.float32, device=dev)
    f = {k: torch.empty((n,) if c == 1 else (n, c), dtype=torch.int32 if ty is np.int32 else torch.float32, device=dev) for k, (ty, c) in abi.SURFACE_FIELDS.items()}
    f2 = {k: torch.empty_like(v) for k, v in f.items()}
    ptr = lambda d, keys=None: {k: v.data_ptr() for k, v in d.items() if keys is None or k in keys}
    print(f"surface at a hit, K3 ground_bunny {W}x{H}: {n} rays; {rounds} rounds of {reps} calls, forms alternating; ms a call")
    print(f"{'rays':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ first':>7s}")
    for name, order in (("row-major", np.arange(n)), ("shuffled", np.random.default_rng(1).permutation(n))):
        d_rays = torch.from_numpy(np.ascontiguousarray(rays[order])).to(dev)
        torch.cuda.synchronize()
        trace = lambda: ds.trace_rays_device(n, d_rays.data_ptr(), stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr())
        full = lambda h, out: (lambda: h.surface_rays_device(n, d_rays.data_ptr(), stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr(), **ptr(out)))
        two = lambda h, out: (lambda: h.surface_rays_device(n, d_rays.data_ptr(), stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr(), **ptr(out, ("normal", "bounce"))))
        trace(); side.synchronize()
        h0, t0 = hit.clone(), t.clone()
        hits = lambda h, out: (lambda: h.surface_hits_device(n, d_rays.data_ptr(), h0.data_ptr(), t0.data_ptr(), stream=cur, **ptr(out)))
        forms = {"trace_rays (k_query_closest)": trace,
                 "surface_rays, all outputs": full(ds, f), "surface_rays, all, lane stores": full(lane, f2),
                 "surface_rays, normal + bounce": two(ds, f), "surface_rays, n + b, lane stores": two(lane, f2),
                 "surface_hits, all outputs": hits(ds, f), "surface_hits, all, lane stores": hits(lane, f2)}
        report(name, rounds_of(forms, reps, rounds, side))
        # the forms answer alike: the two store forms bit for bit, surface_hits as surface_rays, hit ids as the closest-hit query
        full(ds, f)(); full(lane, f2)(); side.synchronize()
        assert torch.equal(hit, h0) and torch.equal(t.view(torch.int32), t0.view(torch.int32))
        assert all(torch.equal(f[k].view(torch.int32), f2[k].view(torch.int32)) for k in f)
        hits(lane, f2)(); side.synchronize()
        assert all(torch.equal(f[k].view(torch.int32), f2[k].view(torch.int32)) for k in f)
        print(f"{'':34s} hits {int((h0 >= 0).sum().item())}; both store forms and surface_hits give the same bits")


def paths_section(reps, rounds):
    """Mirror paths of the 1080p frame, four ways in one run: (a) the chain of existing device calls -- per segment srt_shade_rays_range_device
    and, but for the last, srt_surface_rays_device for the bounce, 2 * depth - 1 launches, with the torch kernels that make the next interval
    and point the rays of ended paths away from the scene --, (b) srt_shade_paths_device on rays built beforehand, (c) srt_render_paths_device, (d) at depth 1, srt_render_device."""
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    n = W * H
    t_min = 1e-3
    d_rays = torch.from_numpy(frame_rays()).to(dev)
    refl = torch.tensor([0.6, 0.25], dtype=torch.float32, device=dev)
    away = torch.tensor([0.0, 0.0, -1e6, 0.0, 0.0, -1.0], dtype=torch.float32, device=dev)      # behind the camera, looking back
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    print(f"mirror paths, K3 ground_bunny {W}x{H}: {n} rays; {rounds} rounds of {reps} calls, forms alternating; ms a call; min / max: the spread of the rounds")
    print(f"{'depth, samples':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ first':>7s}")
    for depth in (1, 3):
        for L in (1, 16):
            lights = abi.light_staircase(g.light, L)
            p = abi.make_params(W, H, lights, focal=FOCAL, flags=abi.SRT_FLAG_NO_TIMING)
            pq = abi.make_params(1, 1, lights)
            lin_a, lin_b, lin_c, lin_d = f32(n, 3), f32(n, 3), f32(H, W, 3), f32(H, W, 3)
            seg_c, nxt, obj, tr = [f32(n, 3) for _ in range(depth)], [f32(n, 6) for _ in range(depth)], i32(n), f32(n, 2)

            def chain():
                with torch.cuda.stream(side):
                    ray, interval = d_rays, None
                    for b in range(depth):
                        ds.shade_rays_device(n, ray.data_ptr(), pq, stream=cur, rgb_linear=seg_c[b].data_ptr(), t_range=interval)
                        if b + 1 < depth:
                            ds.surface_rays_device(n, ray.data_ptr(), stream=cur, obj=obj.data_ptr(), bounce=nxt[b].data_ptr(), t_range=interval)
                            tr[:, 0] = torch.where(obj >= 0, t_min, 1.0)
                            tr[:, 1] = torch.where(obj >= 0, float("inf"), 0.0)
                            nxt[b][obj < 0] = away                 # a path that has ended: a ray that leaves the scene at once (the zero ray of a
                            ray, interval = nxt[b], tr.data_ptr()  # miss row has a NaN slab test and walks every node)

            paths = lambda: ds.shade_paths_device(n, d_rays.data_ptr(), pq, depth, reflectance=refl.data_ptr(), bounce_t_min=t_min, stream=cur, rgb_linear=lin_b.data_ptr())
            frame = lambda: ds.render_paths_device(p, depth, reflectance=refl.data_ptr(), bounce_t_min=t_min, stream=cur, rgb_linear=lin_c.data_ptr())
            forms = {"(a) chain of device calls": chain, "(b) shade_paths_device": paths, "(c) render_paths_device": frame}
            if depth == 1:
                forms["(d) render_device"] = lambda: ds.render_device(p, stream=cur, rgb_linear=lin_d.data_ptr())
            report(f"depth {depth}, {L} samples", rounds_of(forms, reps, rounds, side))
            paths(); frame(); side.synchronize()
            assert torch.equal(lin_b.view(torch.int32), lin_c.view(torch.int32).reshape(n, 3)), "(b) and (c) differ"
            if depth == 1:
                forms["(d) render_device"](); chain(); side.synchronize()
                assert torch.equal(lin_d.view(torch.int32), lin_c.view(torch.int32)) and torch.equal(seg_c[0].view(torch.int32), lin_b.view(torch.int32)), "(a), (d) and (c) differ"
            print(f"{'':34s} (b) and (c) give the same bits" + (", and so do (a) and (d)" if depth == 1 else ""))
    ds.close()


def shadow_rule_section(reps, rounds):
    """What a shadow rule costs srt_shade_paths_device (rays built beforehand) and srt_render_paths_device on the 1080p frame: no rule -- the
    kernels of --paths' (b) and (c) --, shadow rays that end at the light, and those with the hit object's own tree walked too.  The light is
    the scene's far one, so the three shade almost the same pixels: the figures are the cost of the bounded walk, which leaves at the first
    hit IN RANGE instead of the first hit, and of the own tree."""
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    n = W * H
    t_min = 1e-3
    d_rays = torch.from_numpy(frame_rays()).to(dev)
    refl = torch.tensor([0.6, 0.25], dtype=torch.float32, device=dev)
    rules = (("no rule", None), ("(1e-3, 1, 0)", (1e-3, 1.0, False)), ("(1e-3, 1, SELF)", (1e-3, 1.0, True)))
    print(f"shadow rule, K3 ground_bunny {W}x{H}: {n} rays; {rounds} rounds of {reps} calls, forms alternating; ms a call; min / max: the spread of the rounds")
    print(f"{'depth, samples':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ first':>7s}")
    for depth in (1, 3):
        for L in (1, 16):
            lights = abi.light_staircase(g.light, L)
            p = abi.make_params(W, H, lights, focal=FOCAL, flags=abi.SRT_FLAG_NO_TIMING)
            pq = abi.make_params(1, 1, lights)
            lin = {name: (torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((H, W, 3), dtype=torch.float32, device=dev)) for name, _ in rules}
            paths = {f"shade_paths_device, {name}": (lambda rule=rule, out=lin[name][0]: ds.shade_paths_device(
                n, d_rays.data_ptr(), pq, depth, reflectance=refl.data_ptr(), bounce_t_min=t_min, stream=cur, rgb_linear=out.data_ptr(), shadow=rule)) for name, rule in rules}
            frames = {f"render_paths_device, {name}": (lambda rule=rule, out=lin[name][1]: ds.render_paths_device(
                p, depth, reflectance=refl.data_ptr(), bounce_t_min=t_min, stream=cur, rgb_linear=out.data_ptr(), shadow=rule)) for name, rule in rules}
            report(f"depth {depth}, {L} samples", rounds_of(paths, reps, rounds, side))
            report(f"depth {depth}, {L} samples", rounds_of(frames, reps, rounds, side))
            side.synchronize()
            for name, _ in rules:
                assert torch.equal(lin[name][0].view(torch.int32), lin[name][1].view(torch.int32).reshape(n, 3)), f"{name}: the two calls differ"
            diff = {name: int((lin[name][0].view(torch.int32) != lin["no rule"][0].view(torch.int32)).any(dim=1).sum().item()) for name, _ in rules[1:]}
            print(f"{'':34s} both calls give the same bits under every rule; pixels that differ from no rule: {diff}")
    ds.close()


def masked_section(reps, rounds):
    """What one more dependent load per object root costs the walks: the masked calls with all-ones masks beside the calls they extend, on
    the rays of the 1080p frame, and the same calls with the bunny (object 1; object 0 is the ground) hidden."""
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    n = W * H
    t_min = 1e-3
    nO = g.flat.n_objects
    bunny = 1
    ds.set_object_masks((np.uint32(1) << np.arange(nO, dtype=np.uint32)).astype(np.uint32))      # object k carries bit k
    ds.trace_rays(frame_rays()[:1])                                                                # (a host call on the table's stream: it has arrived)
    ALL, NO_BUNNY = 0xFFFFFFFF, 0xFFFFFFFF & ~(1 << bunny)
    d_rays = torch.from_numpy(frame_rays()).to(dev)
    d_open = torch.from_numpy(np.tile(np.float32([0.0, np.inf]), (n, 1))).to(dev)
    d_all = torch.from_numpy(np.full(n, ALL, np.uint32).view(np.int32)).to(dev)
    d_hide = torch.from_numpy(np.full(n, NO_BUNNY, np.uint32).view(np.int32)).to(dev)
    tri_obj = torch.from_numpy(g.flat.tri_obj.astype(np.int64)).to(dev)
    hit = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("range", "ones", "hidden")}
    t = {k: torch.empty(n, dtype=torch.float32, device=dev) for k in hit}
    print(f"visibility masks, K3 ground_bunny {W}x{H}: {n} rays, {nO} objects; {rounds} rounds of {reps} calls, forms alternating; ms a call; min / max: the spread of the rounds")
    print(f"{'call':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ first':>7s}")
    call = lambda key, m: (lambda: ds.trace_rays_device(n, d_rays.data_ptr(), stream=cur, hit_id=hit[key].data_ptr(), t=t[key].data_ptr(), t_range=d_open.data_ptr(), ray_mask=m))
    forms = {"trace_rays_range (yardstick)": call("range", None), "trace_rays_masked, all ones": call("ones", d_all.data_ptr()),
             "trace_rays_masked, NULL ray_mask": call("ones", 0), "trace_rays_masked, bunny hidden": call("hidden", d_hide.data_ptr())}
    report("closest hit, row-major", rounds_of(forms, reps, rounds, side))
    side.synchronize()
    assert torch.equal(hit["range"], hit["ones"]) and torch.equal(t["range"].view(torch.int32), t["ones"].view(torch.int32)), "all ones is not the range call"
    on_bunny = lambda h: int((tri_obj[h.clamp(min=0).long()][h >= 0] == bunny).sum().item())
    assert on_bunny(hit["range"]) > 0 and on_bunny(hit["hidden"]) == 0
    print(f"{'':34s} all ones gives the range call's bits; hits {int((hit['range'] >= 0).sum().item())}, of the bunny {on_bunny(hit['range'])}; with it hidden {int((hit['hidden'] >= 0).sum().item())}")
    refl = torch.tensor([0.6, 0.25], dtype=torch.float32, device=dev)
    rule = (1e-3, 1.0, False)
    for L in (1, 16):
        pq = abi.make_params(1, 1, abi.light_staircase(g.light, L))
        lin = {k: torch.empty((n, 3), dtype=torch.float32, device=dev) for k in ("shadow", "ones", "hidden")}
        paths = lambda key, vis: (lambda: ds.shade_paths_device(n, d_rays.data_ptr(), pq, 3, reflectance=refl.data_ptr(), bounce_t_min=t_min, stream=cur,
                                                                rgb_linear=lin[key].data_ptr(), shadow=rule, visibility=vis))
        forms = {"shade_paths_shadow (yardstick)": paths("shadow", None), "shade_paths_masked, all ones": paths("ones", (ALL, ALL, ALL)),
                 "shade_paths_masked, bunny hidden": paths("hidden", (NO_BUNNY, NO_BUNNY, NO_BUNNY))}
        report(f"paths, depth 3, {L} samples", rounds_of(forms, reps, rounds, side))
        side.synchronize()
        assert torch.equal(lin["shadow"].view(torch.int32), lin["ones"].view(torch.int32)), "all ones is not the _shadow call"
        diff = int((lin["hidden"].view(torch.int32) != lin["shadow"].view(torch.int32)).any(dim=1).sum().item())
        print(f"{'':34s} all ones gives the _shadow call's bits; pixels the hidden bunny changes: {diff}")
    ds.close()


def refract_section(reps, rounds):
    """What the REFRACT build costs: the _refract call with an all-zero table beside the _masked call it extends (the same walks, the
    same bits), on the rays of the 1080p frame at depth 3; and the same call with the bunny (object 1; object 0 is the ground) as glass."""
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    n = W * H
    nO = g.flat.n_objects
    ALL = 0xFFFFFFFF
    d_rays = torch.from_numpy(frame_rays()).to(dev)
    refl = torch.tensor([0.6, 0.25], dtype=torch.float32, device=dev)
    d_zero = torch.zeros(nO, dtype=torch.float32, device=dev)
    d_glass = torch.tensor([0.0, 1.5], dtype=torch.float32, device=dev)
    rule, vis = (1e-3, 1.0, False), (ALL, ALL, ALL)
    print(f"refracting paths, K3 ground_bunny {W}x{H}: {n} rays, {nO} objects, depth 3; {rounds} rounds of {reps} calls, forms alternating; ms a call; min / max: the spread of the rounds")
    print(f"{'call':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ first':>7s}")
    for L in (1, 16):
        pq = abi.make_params(1, 1, abi.light_staircase(g.light, L))
        lin = {k: torch.empty((n, 3), dtype=torch.float32, device=dev) for k in ("masked", "zero", "glass")}
        hit = {k: torch.empty((3, n), dtype=torch.int32, device=dev) for k in lin}
        paths = lambda key, table: (lambda: ds.shade_paths_device(n, d_rays.data_ptr(), pq, 3, reflectance=refl.data_ptr(), bounce_t_min=1e-3, stream=cur,
                                                                  rgb_linear=lin[key].data_ptr(), seg_hit_id=hit[key].data_ptr(), shadow=rule, visibility=vis, ior=table))
        forms = {"shade_paths_masked (yardstick)": paths("masked", None), "shade_paths_refract, all zero": paths("zero", d_zero.data_ptr()),
                 "shade_paths_refract, glass bunny": paths("glass", d_glass.data_ptr())}
        ms = rounds_of(forms, reps, rounds, side)
        report(f"paths, depth 3, {L} samples", ms)
        side.synchronize()
        assert torch.equal(lin["masked"].view(torch.int32), lin["zero"].view(torch.int32)) and torch.equal(hit["masked"], hit["zero"]), "all zero is not the _masked call"
        yard = ms["shade_paths_masked (yardstick)"]
        med = float(np.median(yard))
        moved = int((hit["glass"] != hit["masked"]).any(dim=0).sum().item())
        print(f"{'':34s} all zero gives the _masked call's bits; the yardstick's own spread: {min(yard) / med:.3f} .. {max(yard) / med:.3f} of its median; "
              f"hits per segment, mirror {[int((hit['masked'][b] >= 0).sum().item()) for b in range(3)]}, glass {[int((hit['glass'][b] >= 0).sum().item()) for b in range(3)]}; "
              f"paths the glass moves: {moved}")
    ds.close()


def fresnel_section(reps, rounds):
    """What the Fresnel split costs srt_shade_paths_refract_device on the rays of the 1080p frame at depth 3 with the bunny (object 1) as
    glass of index 1.5: (a) the _fresnel call with an all-negative f0 -- nothing splits, the same bits: the price of the build alone --,
    (b) with f0 = schlick_f0(ior): the price of the side walks, beside the chain of device calls that computes the same pixels -- the
    _refract call with seg, and per segment srt_surface_hits_device for normal and bounce row, torch for who splits, F and the
    compaction of the side rays, the depth-1 _masked call on them, and the mix in torch."""
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    n, D = W * H, 3
    ALL = 0xFFFFFFFF
    f32, i32 = torch.float32, torch.int32
    d_rays = torch.from_numpy(frame_rays()).to(dev)
    refl_h = np.float32([0.6, 0.25])
    refl = torch.from_numpy(refl_h).to(dev)
    ior_h = np.float32([0.0, 1.5])
    d_ior = torch.from_numpy(ior_h).to(dev)
    d_neg = torch.full((2,), -1.0, dtype=f32, device=dev)
    d_f0 = torch.from_numpy(lib.schlick_f0(ior_h)).to(dev)
    rule, vis = (1e-3, 1.0, False), (ALL, ALL, ALL)
    print(f"Fresnel split, K3 ground_bunny {W}x{H}: {n} rays, 2 objects, depth {D}; {rounds} rounds of {reps} calls, forms alternating; ms a call; min / max: the spread of the rounds")
    print(f"{'call':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ first':>7s}")
    for L in (1, 16):
        pq = abi.make_params(1, 1, abi.light_staircase(g.light, L))
        keys = ("refract", "negative", "split", "chain")
        lin = {k: torch.empty((n, 3), dtype=f32, device=dev) for k in keys}
        hit = {k: torch.empty((D, n), dtype=i32, device=dev) for k in keys}
        F_rows = torch.zeros((D, n), dtype=f32, device=dev)
        s_hit = torch.full((D, n), -1, dtype=i32, device=dev)
        paths = lambda key, f0: (lambda: ds.shade_paths_device(n, d_rays.data_ptr(), pq, D, reflectance=refl.data_ptr(), bounce_t_min=1e-3, stream=cur,
                                                               rgb_linear=lin[key].data_ptr(), seg_hit_id=hit[key].data_ptr(), shadow=rule, visibility=vis, ior=d_ior.data_ptr(),
                                                               fresnel=f0, side_hit_id=s_hit.data_ptr() if key == "split" else 0,
                                                               side_fresnel=F_rows.data_ptr() if key == "split" else 0))
        # the chain's buffers
        seg_t = torch.empty((D, n), dtype=f32, device=dev); seg_obj = torch.empty((D, n), dtype=i32, device=dev)
        seg_lin = torch.empty((D, n, 3), dtype=f32, device=dev); seg_rays = torch.empty((D, n, 6), dtype=f32, device=dev)
        nrm = torch.empty((n, 3), dtype=f32, device=dev); bounce = torch.empty((n, 6), dtype=f32, device=dev)
        c_hit = torch.empty(n, dtype=i32, device=dev); c_lin = torch.empty((n, 3), dtype=f32, device=dev)

        def chain():
            with torch.cuda.stream(side):
                ds.shade_paths_device(n, d_rays.data_ptr(), pq, D, reflectance=refl.data_ptr(), bounce_t_min=1e-3, stream=cur, seg_hit_id=hit["chain"].data_ptr(),
                                      seg_t=seg_t.data_ptr(), seg_obj=seg_obj.data_ptr(), seg_rgb_linear=seg_lin.data_ptr(), seg_rays=seg_rays.data_ptr(), shadow=rule,
                                      visibility=vis, ior=d_ior.data_ptr())
                acc, Wt = torch.zeros((n, 3), dtype=f32, device=dev), torch.ones(n, dtype=f32, device=dev)
                going = torch.ones(n, dtype=torch.bool, device=dev)
                for b in range(D):
                    going = going & (hit["chain"][b] >= 0)
                    nxt = going & (hit["chain"][b + 1] >= 0) if b + 1 < D else torch.zeros_like(going)
                    obj = seg_obj[b].clamp(min=0).long()
                    sd = torch.zeros_like(going); Ssum = torch.zeros((n, 3), dtype=f32, device=dev); Fb = torch.zeros(n, dtype=f32, device=dev)
                    if b + 1 < D:
                        ds.surface_hits_device(n, seg_rays[b].data_ptr(), hit["chain"][b].data_ptr(), seg_t[b].data_ptr(), stream=cur, normal=nrm.data_ptr(),
                                               bounce=bounce.data_ptr())
                        d = seg_rays[b][:, 3:6]
                        Ln = torch.sqrt((d * d).sum(1)); I = d / Ln[:, None]
                        c = (nrm * I).sum(1)
                        ent = c < 0
                        dv = torch.where(ent, c, -c)
                        nn = d_ior[obj]
                        eta = torch.where(ent, 1.0 / nn, nn)
                        k = 1.0 - (eta * eta) * (1.0 - dv * dv)
                        walked = going & (nn > 0) & (d_f0[obj] >= 0) & ~(k < 0)
                        x = torch.where(ent, -dv, torch.sqrt(k)); m = 1.0 - x; m2 = m * m
                        Fb = torch.where(walked, d_f0[obj] + (1.0 - d_f0[obj]) * ((m2 * m2) * m), Fb)
                        idx = torch.nonzero(walked).squeeze(1)
                        ns = int(idx.numel())      # (a host sync: the chain needs the count)
                        if ns:
                            srays = bounce.index_select(0, idx).contiguous()
                            tr = torch.tensor([1e-3, float("inf")], dtype=f32, device=dev).repeat(ns, 1).contiguous()
                            ds.shade_paths_device(ns, srays.data_ptr(), pq, 1, bounce_t_min=1e-3, t_range=tr.data_ptr(), stream=cur, rgb_linear=0,
                                                  seg_hit_id=c_hit.data_ptr(), seg_rgb_linear=c_lin.data_ptr(), shadow=rule, visibility=vis)
                            sd[idx] = c_hit[:ns] >= 0
                            Ssum[idx] = c_lin[:ns]
                    kk = torch.where(nxt | sd, refl[obj], torch.zeros(n, dtype=f32, device=dev))
                    a = Wt * (1.0 - kk)
                    acc = torch.where(going[:, None], acc + a[:, None] * seg_lin[b], acc)
                    Wk = Wt * kk
                    Fe = torch.where(sd, torch.where(nxt, Fb, torch.ones_like(Fb)), torch.zeros_like(Fb))
                    acc = torch.where(sd[:, None], acc + (Wk * Fe)[:, None] * Ssum, acc)
                    Wt = torch.where(going, Wk * (1.0 - Fe), Wt)
                lin["chain"].copy_(acc)

        forms = {"shade_paths_refract (yardstick)": paths("refract", None), "shade_paths_fresnel, f0 all -1": paths("negative", d_neg.data_ptr()),
                 "shade_paths_fresnel, f0 0.04": paths("split", d_f0.data_ptr()), "chain of device calls": chain}
        ms = rounds_of(forms, reps, rounds, side)
        report(f"paths, depth {D}, {L} samples", ms)
        side.synchronize()
        assert torch.equal(lin["refract"].view(i32), lin["negative"].view(i32)) and torch.equal(hit["refract"], hit["negative"]), "no split is not the _refract call"
        assert torch.equal(hit["refract"], hit["split"]), "the split moved a segment"
        differ = int((lin["chain"].view(i32) != lin["split"].view(i32)).any(dim=1).sum().item())
        worst = float((lin["chain"] - lin["split"]).abs().max().item())
        yard = ms["shade_paths_refract (yardstick)"]
        med = float(np.median(yard))
        # the lanes of the side walks: F > 0 marks a side ray (f0 = 0.04); waves by the deal the call used
        walked = (F_rows > 0).cpu().numpy()
        n_waves = ((n + 255) // 256) * 4
        pad = np.zeros((D, n_waves * 64), bool); pad[:, :n] = walked
        per_wave = pad.reshape(D, 8, n_waves, 8).sum(axis=(1, 3)) if L >= 8 else pad.reshape(D, n_waves, 64).sum(axis=2)
        share = [float(per_wave[b].sum() / (64.0 * max(1, (per_wave[b] > 0).sum()))) for b in range(D - 1)]
        print(f"{'':34s} f0 all -1 gives the _refract call's bits; the yardstick's own spread: {min(yard) / med:.3f} .. {max(yard) / med:.3f} of its median; "
              f"side rays walked per segment {[int(walked[b].sum()) for b in range(D)]}, that hit {[int((s_hit[b] >= 0).sum().item()) for b in range(D)]}; "
              f"waves that walk side rays {[int((per_wave[b] > 0).sum()) for b in range(D - 1)]} of {n_waves}, share of their lanes active {[round(x, 3) for x in share]}; "
              f"chain against the one launch: {differ} pixels differ in a bit, at most {worst:.3g} (torch rounds the glue on its own)")
    ds.close()


def ao_section(reps, rounds):
    from simple_raytracer_amd import build
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    handles = {"shipped rule": lib.DeviceScene(g.flat), "spread deal": lib.DeviceScene(g.flat, library=lib.load(build.build_ao_deal(True))),
               "block deal": lib.DeviceScene(g.flat, library=lib.load(build.build_ao_deal(False)))}
    ds = handles["shipped rule"]
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    rays = frame_rays()
    n = rays.shape[0]
    t_min, t_max = 1e-3, 60.0
    d_rays = torch.from_numpy(rays).to(dev)
    frame = ds.render(g.params(W, H, 1), want=("hit_id", "t"))
    h0, t0 = torch.from_numpy(frame["hit_id"].reshape(-1).copy()).to(dev), torch.from_numpy(frame["t"].reshape(-1).copy()).to(dev)
    hit = torch.empty(n, dtype=torch.int32, device=dev); t = torch.empty(n, dtype=torch.float32, device=dev)
    point, normal = torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev)
    print(f"ambient occlusion, K3 ground_bunny {W}x{H}: {n} rays, {int((h0 >= 0).sum().item())} hits, t in ({t_min}, {t_max}); {rounds} rounds of {reps} calls, forms "
          f"alternating; ms a call; min / max: the spread of the rounds")
    print(f"{'directions':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ chain':>7s}")
    for K in (16, 64):
        d_dirs = torch.from_numpy(lib.ao_directions(K)).to(dev)
        cnt = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("chain", "rays", "hits")}
        ao = {k: torch.empty(n, dtype=torch.float32, device=dev) for k in cnt}
        aor = torch.empty((n, K, 6), dtype=torch.float32, device=dev)
        mask = torch.empty((n, K), dtype=torch.int32, device=dev)
        occ = torch.empty((n, K), dtype=torch.uint8, device=dev)
        tr = torch.tensor([t_min, t_max], dtype=torch.float32, device=dev).repeat(n * K, 1).contiguous()
        torch.cuda.synchronize()

        def chain():
            with torch.cuda.stream(side):
                ds.surface_rays_device(n, d_rays.data_ptr(), stream=cur, hit_id=hit.data_ptr(), point=point.data_ptr(), normal=normal.data_ptr())
                d = d_rays[:, 3:6]
                k = (d[:, 0] * normal[:, 0] + d[:, 1] * normal[:, 1]) + d[:, 2] * normal[:, 2]
                Nf = torch.where((k > 0)[:, None], -normal, normal)
                x, y, z = Nf[:, 0], Nf[:, 1], Nf[:, 2]
                s = torch.copysign(torch.ones_like(z), z)
                a = -1.0 / (s + z)
                b = (x * y) * a
                T = torch.stack([1.0 + ((s * x) * x) * a, s * b, (-s) * x], dim=1)
                B = torch.stack([b, s + (y * y) * a, -y], dim=1)
                aor[:, :, 0:3] = point[:, None, :]
                aor[:, :, 3:6] = (T[:, None, :] * d_dirs[None, :, 0:1] + B[:, None, :] * d_dirs[None, :, 1:2]) + Nf[:, None, :] * d_dirs[None, :, 2:3]
                mask[:] = torch.where(hit >= 0, -1, 0)[:, None]
                ds.occluded_device(n * K, aor.data_ptr(), occ.data_ptr(), stream=cur, t_range=tr.data_ptr(), ray_mask=mask.data_ptr())
                torch.sum(occ, dim=1, dtype=torch.int32, out=cnt["chain"])
                torch.div((K - cnt["chain"]).to(torch.float32), float(K), out=ao["chain"])

        fused = lambda h: (lambda: h.ao_rays_device(n, d_rays.data_ptr(), d_dirs.data_ptr(), K, t_min, t_max, stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr(),
                                                    n_occluded=cnt["rays"].data_ptr(), ao=ao["rays"].data_ptr()))
        on_hits = lambda h: (lambda: h.ao_hits_device(n, d_rays.data_ptr(), h0.data_ptr(), t0.data_ptr(), d_dirs.data_ptr(), K, t_min, t_max, stream=cur,
                                                      n_occluded=cnt["hits"].data_ptr(), ao=ao["hits"].data_ptr()))
        forms = {"chain (yardstick)": chain}
        forms.update({f"ao_rays_device, {name}": fused(h) for name, h in handles.items()})
        forms.update({f"ao_hits_device, {name}": on_hits(h) for name, h in handles.items()})
        report(f"{K} directions", rounds_of(forms, reps, rounds, side))
        # every form answers alike
        chain(); side.synchronize()
        for name, h in handles.items():
            cnt["rays"].fill_(-1); cnt["hits"].fill_(-1)
            fused(h)(); on_hits(h)(); side.synchronize()
            assert torch.equal(hit, h0) and torch.equal(t.view(torch.int32), t0.view(torch.int32)), name
            for k in ("rays", "hits"):
                assert torch.equal(cnt[k], cnt["chain"]) and torch.equal(ao[k].view(torch.int32), ao["chain"].view(torch.int32)), (name, k)
        print(f"{'':34s} blocked {int(cnt['chain'].sum().item())} of {int((h0 >= 0).sum().item()) * K} AO rays; the chain, both calls and both deals give the same bits")
    for h in handles.values():
        h.close()


def render_ao_section(reps, rounds):
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    p = g.params(W, H, 1)
    n = W * H
    t_min, t_max = 1e-3, 60.0
    frame = ds.render(p, want=("hit_id", "t"))
    h0, t0 = torch.from_numpy(frame["hit_id"].reshape(-1).copy()).to(dev), torch.from_numpy(frame["t"].reshape(-1).copy()).to(dev)
    i0, j0 = int(-np.float32(W) / 2), int(-np.float32(H) / 2)
    xs = torch.arange(i0, i0 + W, dtype=torch.float32, device=dev); ys = torch.arange(j0, j0 + H, dtype=torch.float32, device=dev)
    d_rays = torch.zeros((H, W, 6), dtype=torch.float32, device=dev)
    hit = torch.empty(n, dtype=torch.int32, device=dev); t = torch.empty(n, dtype=torch.float32, device=dev)
    rot = lib.ao_rotations(4, 4)
    d_rot = torch.from_numpy(rot).to(dev)
    turned = dict(rot=d_rot.data_ptr(), rot_w=4, rot_h=4)
    names = ("shipped", "frame", "turned", "bent")
    cnt = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in names}
    ao = {k: torch.empty(n, dtype=torch.float32, device=dev) for k in names}
    bent = torch.empty((n, 3), dtype=torch.float32, device=dev)
    print(f"ambient occlusion in a frame, K3 ground_bunny {W}x{H}: {n} pixels, {int((h0 >= 0).sum().item())} hits, t in ({t_min}, {t_max}); {rounds} rounds of {reps} calls, "
          f"forms alternating; ms a call; min / max: the spread of the rounds")
    print(f"{'directions':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ first':>7s}")

    def make_rays():      # what a caller of the ray forms does per frame: 24 B a pixel, written here by four elementwise launches
        with torch.cuda.stream(side):
            d_rays[..., 0:3] = 0.0
            d_rays[..., 3] = xs[None, :]
            d_rays[..., 4] = ys[:, None]
            d_rays[..., 5] = FOCAL

    for K in (16, 64):
        d_dirs = torch.from_numpy(lib.ao_directions(K)).to(dev)
        torch.cuda.synchronize()
        outs = lambda k: dict(n_occluded=cnt[k].data_ptr(), ao=ao[k].data_ptr())

        def shipped_rays():
            make_rays()
            ds.ao_rays_device(n, d_rays.data_ptr(), d_dirs.data_ptr(), K, t_min, t_max, stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr(), **outs("shipped"))

        def shipped_hits():
            make_rays()
            ds.ao_hits_device(n, d_rays.data_ptr(), h0.data_ptr(), t0.data_ptr(), d_dirs.data_ptr(), K, t_min, t_max, stream=cur, **outs("shipped"))

        ray_form = lambda k, **kw: (lambda: ds.render_ao_device(p, d_dirs.data_ptr(), K, t_min=t_min, t_max=t_max, stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr(),
                                                                **outs(k), **kw))
        hits_form = lambda k, **kw: (lambda: ds.render_ao_hits_device(p, h0.data_ptr(), t0.data_ptr(), d_dirs.data_ptr(), K, t_min=t_min, t_max=t_max, stream=cur,
                                                                      **outs(k), **kw))
        for title, first, form in ((f"{K} directions, the hit found", shipped_rays, ray_form), (f"{K} directions, a render's hits", shipped_hits, hits_form)):
            kind = "ao_rays" if form is ray_form else "ao_hits"
            own = "render_ao_device" if form is ray_form else "render_ao_hits_device"
            forms = {f"torch rays + {kind}_device (yardstick)": first, own: form("frame"), f"{own}, 4x4 rot": form("turned", **turned),
                     f"{own}, 4x4 rot, bent": form("bent", **turned, bent=bent.data_ptr())}
            report(title, rounds_of(forms, reps, rounds, side))
            # the frame form without a table answers as the shipped call; the table changes rows; bent changes nothing else
            for k in names:
                cnt[k].fill_(-1)
            for fn in forms.values():
                fn()
            side.synchronize()
            assert torch.equal(cnt["frame"], cnt["shipped"]) and torch.equal(ao["frame"].view(torch.int32), ao["shipped"].view(torch.int32)), title
            assert torch.equal(cnt["bent"], cnt["turned"]) and not torch.equal(cnt["turned"], cnt["frame"]), title
            if form is ray_form:
                assert torch.equal(hit, h0) and torch.equal(t.view(torch.int32), t0.view(torch.int32)), title
        print(f"{'':34s} blocked {int(cnt['frame'].sum().item())} of {int((h0 >= 0).sum().item()) * K} AO rays without the table, {int(cnt['turned'].sum().item())} with it; "
              f"the frame forms without a table give the shipped calls' bits")
    ds.close()


def points_section(reps, rounds, nearest=False):
    """What a closest-point walk costs beside a ray's: the hit points of the 1080p frame, OFFSETS units off the surface towards the camera,
    with RADII on every STEP-th hit and with no radius on every (16 STEP)-th, each beside srt_trace_rays_device on the rays of the same pixels.
    nearest: srt_nearest_points_device beside srt_closest_points_device, the yardstick, on the same points in the same rounds, radius by
    radius: the ratio of the medians, and both calls' node and triangle tests per point."""
    OFFSETS, RADII, STEP = (0.25, 2.0, 16.0), (1.0, 4.0, 16.0, 64.0), 4
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    rays = frame_rays()
    frame = ds.trace_rays(rays, want=("hit_id", "t"))
    hits = np.flatnonzero(frame["hit_id"] >= 0)
    P = rays[hits, 3:6] * frame["t"][hits, None]                      # (the origin is 0)
    unit = rays[hits, 3:6] / np.linalg.norm(rays[hits, 3:6], axis=1, keepdims=True)
    print(f"closest points, K3 ground_bunny {W}x{H}: {g.flat.n_tris} triangles, {g.flat.n_nodes} nodes; {hits.size} hit points; {rounds} rounds of {reps} calls, forms "
          f"alternating; ms a call; min / max: the spread of the rounds")
    for step, radii in ((STEP, RADII), (16 * STEP, (np.inf,))):
        sel = np.arange(0, hits.size, step)
        n = sel.size
        d_rays = torch.from_numpy(np.ascontiguousarray(rays[hits[sel]])).to(dev)
        hit, t = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        tri, d2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        pt = torch.empty((n, 3), dtype=torch.float32, device=dev)
        print(f"every {step}th hit: {n} points, {n} rays")
        print(f"{'points':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ first':>7s}")
        for off in OFFSETS:
            pts = np.ascontiguousarray(P[sel] - unit[sel] * np.float32(off), np.float32)
            d_pts = torch.from_numpy(pts).to(dev)
            d_rad = {r: torch.full((n,), float(r), dtype=torch.float32, device=dev) for r in radii}
            forms = {"trace_rays (yardstick)": lambda: ds.trace_rays_device(n, d_rays.data_ptr(), stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr())}
            for r in radii:
                forms[f"closest_points, radius {r:g}"] = (lambda r=r: ds.closest_points_device(n, d_pts.data_ptr(), radius=0 if np.isinf(r) else d_rad[r].data_ptr(), stream=cur,
                                                                                               tri=tri.data_ptr(), dist2=d2.data_ptr(), point=pt.data_ptr()))
            if nearest:
                forms = {}
                for r in radii:
                    for call in ("closest_points", "nearest_points"):
                        forms[f"{call}, radius {r:g}"] = (lambda r=r, fn=getattr(ds, call + "_device"): fn(n, d_pts.data_ptr(), radius=0 if np.isinf(r) else d_rad[r].data_ptr(),
                                                                                                          stream=cur, tri=tri.data_ptr(), dist2=d2.data_ptr(), point=pt.data_ptr()))
                ms = rounds_of(forms, reps, rounds, side)
                side.synchronize()
                for r in radii:
                    pair = {k: ms[f"{k}, radius {r:g}"] for k in ("closest_points", "nearest_points")}
                    report(f"{off:g} off the surface, radius {r:g}", pair)
                    both = {k: getattr(ds, k)(pts, radius=None if np.isinf(r) else r, count=True, want=("tri", "dist2")) for k in pair}
                    assert all(np.array_equal(both["closest_points"][k].view(np.uint32), both["nearest_points"][k].view(np.uint32)) for k in ("tri", "dist2"))
                    for k, o in both.items():
                        print(f"{'':34s} {k}: found {int((o['tri'] >= 0).sum())} of {n}; per point {o['stats']['node_tests_primary'] / n:.1f} node tests, "
                              f"{o['stats']['tri_tests_primary'] / n:.1f} triangle tests")
                continue
            report(f"{off:g} off the surface", rounds_of(forms, reps, rounds, side))
            side.synchronize()
            for r in radii:
                o = ds.closest_points(pts, radius=None if np.isinf(r) else r, count=True, want=("tri", "dist2"))
                st = o["stats"]
                found = o["tri"] >= 0
                print(f"{'':34s} radius {r:g}: found {int(found.sum())} of {n}, median distance {float(np.sqrt(np.median(o['dist2'][found]))) if found.any() else float('nan'):.3f}; "
                      f"per point {st['node_tests_primary'] / n:.1f} node tests, {st['tri_tests_primary'] / n:.1f} triangle tests")
            st = ds.trace_rays(rays[hits[sel]], count=True, want=())["stats"]
            print(f"{'':34s} the rays: per ray {st['node_tests_primary'] / n:.1f} node tests, {st['tri_tests_primary'] / n:.1f} triangle tests")
    ds.close()


def points_multi_section(reps, rounds):
    """The K nearest triangles per point (srt_closest_points_multi_device, srt_nearest_points_multi_device; k = 1, 4, 16) beside the
    single-winner calls srt_closest_points_device and srt_nearest_points_device, in the same rounds: the points of --nearest -- the hit
    points of the 1080p frame OFFSETS units off the surface, radii RADII on every STEP-th hit, no radius on every (16 STEP)-th.  Written:
    n_found, tri, dist2 (the single-winner calls: tri, dist2).  The spread of the single-winner calls across the rounds is the noise floor;
    k = 1 against them is the price of the slots.  Equal bits of column 0 are asserted, and the counters are printed: the closest form's are
    srt_closest_points', the nearest form's lie below them."""
    OFFSETS, RADII, STEP, KS = (0.25, 2.0), (1.0, 4.0, 16.0), 4, (1, 4, 16)
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    rays = frame_rays()
    frame = ds.trace_rays(rays, want=("hit_id", "t"))
    hits = np.flatnonzero(frame["hit_id"] >= 0)
    P = rays[hits, 3:6] * frame["t"][hits, None]                      # (the origin is 0)
    unit = rays[hits, 3:6] / np.linalg.norm(rays[hits, 3:6], axis=1, keepdims=True)
    print(f"K nearest triangles per point, K3 ground_bunny {W}x{H}: {g.flat.n_tris} triangles, {g.flat.n_nodes} nodes; {hits.size} hit points; {rounds} rounds of {reps} "
          f"calls, forms alternating; ms a call; min / max: the spread of the rounds; / first: over srt_closest_points_device")
    for step, radii in ((STEP, RADII), (16 * STEP, (np.inf,))):
        sel = np.arange(0, hits.size, step)
        n = sel.size
        tri, d2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        nf = torch.empty(n, dtype=torch.int32, device=dev)
        mtri, md2 = torch.empty((n, max(KS)), dtype=torch.int32, device=dev), torch.empty((n, max(KS)), dtype=torch.float32, device=dev)
        print(f"every {step}th hit: {n} points")
        print(f"{'points':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ first':>7s}")
        for off in OFFSETS:
            pts = np.ascontiguousarray(P[sel] - unit[sel] * np.float32(off), np.float32)
            d_pts = torch.from_numpy(pts).to(dev)
            for r in radii:
                d_rad = 0 if np.isinf(r) else torch.full((n,), float(r), dtype=torch.float32, device=dev)
                rad = 0 if np.isinf(r) else d_rad.data_ptr()
                forms = {}
                for call in ("closest_points", "nearest_points"):
                    forms[call] = (lambda fn=getattr(ds, call + "_device"): fn(n, d_pts.data_ptr(), radius=rad, stream=cur, tri=tri.data_ptr(), dist2=d2.data_ptr()))
                for k in KS:
                    for call in ("closest_points_multi", "nearest_points_multi"):
                        forms[f"{call}, k {k}"] = (lambda k=k, fn=getattr(ds, call + "_device"): fn(n, d_pts.data_ptr(), k, radius=rad, stream=cur, n_found=nf.data_ptr(),
                                                                                                  tri=mtri.data_ptr(), dist2=md2.data_ptr()))
                report(f"{off:g} off the surface, radius {r:g}", rounds_of(forms, reps, rounds, side))
                side.synchronize()
                host_r = None if np.isinf(r) else r
                one = ds.closest_points(pts, radius=host_r, count=True, want=("tri", "dist2"))
                print(f"{'':34s} closest_points: found {int((one['tri'] >= 0).sum())} of {n}; per point {one['stats']['node_tests_primary'] / n:.1f} node tests, "
                      f"{one['stats']['tri_tests_primary'] / n:.1f} triangle tests")
                for k in KS:
                    close = ds.closest_points_multi(pts, k, radius=host_r, count=True, want=("n_within", "n_found", "tri", "dist2"))
                    near = ds.nearest_points_multi(pts, k, radius=host_r, count=True, want=("n_found", "tri", "dist2"))
                    assert all(np.array_equal(close[key].view(np.uint32), near[key].view(np.uint32)) for key in ("n_found", "tri", "dist2"))
                    assert all(np.array_equal(close[key][:, 0].view(np.uint32), one[key].view(np.uint32)) for key in ("tri", "dist2"))
                    a, b = close["stats"], near["stats"]
                    assert (a["node_tests_primary"], a["tri_tests_primary"]) == (one["stats"]["node_tests_primary"], one["stats"]["tri_tests_primary"])
                    assert b["node_tests_primary"] <= a["node_tests_primary"] and b["tri_tests_primary"] <= a["tri_tests_primary"]
                    print(f"{'':34s} k {k}: within the radius, median {int(np.median(close['n_within']))}, mean found {close['n_found'].mean():.2f}; per point, closest form "
                          f"{a['node_tests_primary'] / n:.1f} node / {a['tri_tests_primary'] / n:.1f} triangle tests, nearest form {b['node_tests_primary'] / n:.1f} / "
                          f"{b['tri_tests_primary'] / n:.1f}")
    ds.close()


def signed_section(reps, rounds):
    """srt_signed_points_device beside the chain of shipped calls it replaces, beside srt_nearest_points_device alone, and containment only:
    the hit points of the 1080p frame OFFSETS units off the surface towards the camera, every STEP-th and every (16 STEP)-th as in --nearest,
    and all of them (the one batch here that fills the machine more than once), no radius."""
    OFFSETS, STEP = (0.25, 2.0, 16.0), 4
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    rays = frame_rays()
    frame = ds.trace_rays(rays, want=("hit_id", "t"))
    hits = np.flatnonzero(frame["hit_id"] >= 0)
    P = rays[hits, 3:6] * frame["t"][hits, None]                      # (the origin is 0)
    unit = rays[hits, 3:6] / np.linalg.norm(rays[hits, 3:6], axis=1, keepdims=True)
    d_dirs = torch.from_numpy(abi.SIGN_DEFAULT_DIRS).to(dev)
    print(f"signed distance, K3 ground_bunny {W}x{H}: {g.flat.n_tris} triangles, {g.flat.n_nodes} nodes; {hits.size} hit points; 3 directions, parity; no radius; "
          f"{rounds} rounds of {reps} calls, forms alternating; ms a call; min / max: the spread of the rounds")
    for step in (1, STEP, 16 * STEP):
        sel = np.arange(0, hits.size, step)
        n = sel.size
        new = lambda shape, ty: torch.empty(shape, dtype=ty, device=dev)
        s_tri, s_d2, s_pt, s_sd, s_in = new(n, torch.int32), new(n, torch.float32), new((n, 3), torch.float32), new(n, torch.float32), new(n, torch.uint8)
        c_tri, c_d2, c_pt, c_nh, c_rays = new(n, torch.int32), new(n, torch.float32), new((n, 3), torch.float32), new((n, 3), torch.int32), new((n, 3, 6), torch.float32)
        only = new(n, torch.uint8)
        kept = {}
        print(f"every {step}th hit: {n} points" if step > 1 else f"every hit: {n} points")
        print(f"{'points':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ first':>7s}")
        for off in OFFSETS:
            pts = np.ascontiguousarray(P[sel] - unit[sel] * np.float32(off), np.float32)
            d_pts = torch.from_numpy(pts).to(dev)
            torch.cuda.synchronize()

            def chain():
                ds.nearest_points_device(n, d_pts.data_ptr(), stream=cur, tri=c_tri.data_ptr(), dist2=c_d2.data_ptr(), point=c_pt.data_ptr())
                with torch.cuda.stream(side):
                    c_rays[:, :, :3] = d_pts[:, None, :]
                    c_rays[:, :, 3:] = d_dirs[None, :, :]
                ds.trace_rays_multi_device(3 * n, c_rays.data_ptr(), 1, stream=cur, n_hits=c_nh.data_ptr())
                with torch.cuda.stream(side):
                    inside = 2 * (c_nh & 1).sum(1) > 3
                    root = torch.sqrt(c_d2)
                    kept["inside"], kept["sdist"] = inside.to(torch.uint8), torch.where(inside, -root, root)
            forms = {
                "chain of shipped calls": chain,
                "signed_points, one launch": lambda: ds.signed_points_device(n, d_pts.data_ptr(), parity=True, stream=cur, tri=s_tri.data_ptr(), dist2=s_d2.data_ptr(),
                                                                             point=s_pt.data_ptr(), sdist=s_sd.data_ptr(), inside=s_in.data_ptr()),
                "nearest_points alone": lambda: ds.nearest_points_device(n, d_pts.data_ptr(), stream=cur, tri=c_tri.data_ptr(), dist2=c_d2.data_ptr(), point=c_pt.data_ptr()),
                "signed_points, containment only": lambda: ds.signed_points_device(n, d_pts.data_ptr(), parity=True, stream=cur, inside=only.data_ptr()),
            }
            ms = rounds_of(forms, reps, rounds, side)
            side.synchronize()
            report(f"{off:g} off the surface", ms)
            same = all(torch.equal(a, b) for a, b in ((s_tri, c_tri), (s_d2.view(torch.int32), c_d2.view(torch.int32)), (s_pt.view(torch.int32), c_pt.view(torch.int32)),
                                                      (s_in, kept["inside"]), (s_sd.view(torch.int32), kept["sdist"].view(torch.int32)), (only, s_in)))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            c = ms["chain of shipped calls"]
            print(f"{'':34s} equal bits: {same}; inside {int(s_in.sum().item())} of {n}; the chain's own spread {(max(c) - min(c)) / med['chain of shipped calls'] * 100:.1f} % of its median; "
                  f"the sign on top of nearest_points {med['signed_points, one launch'] - med['nearest_points alone']:.3f} ms; containment only "
                  f"{med['signed_points, containment only'] * 1e6 / n:.1f} ns a point")
            assert same
    ds.close()


def segments_section(reps, rounds):
    """What a segment walk costs (srt_closest_segments_device): the hit points of the 1080p frame, 0.25 off the surface towards the camera,
    every 64th of them (12,270, the sample tools/ray_query_probe.py --nearest walks without a radius) and every 4th (196,319, its sample with radii).
    (a) point segments (B = A) beside srt_closest_points_device at the same radii: the price of the policy itself.
    (b) segments of length L in random directions with the point as their midpoint, radius r, beside what a caller could do before:
    srt_closest_points_device at the midpoint with radius r + L / 2 (a ball that holds the capsule; it answers another question).
    (c) the same segments through the library built without box test 2 (python -m simple_raytracer_amd.build --segments-no-box-test-2), when
    that build is there: what the test buys on sloped segments.  Written: tri, dist2, s (the point calls: tri, dist2)."""
    from simple_raytracer_amd import build
    OFF = 0.25
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    other = lib.DeviceScene(g.flat, library=lib.load(build.LIB_SEGMENTS_NO_BOX_TEST_2)) if os.path.exists(build.LIB_SEGMENTS_NO_BOX_TEST_2) else None
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    rays = frame_rays()
    frame = ds.trace_rays(rays, want=("hit_id", "t"))
    hits = np.flatnonzero(frame["hit_id"] >= 0)
    for STEP in (64, 4):
        sel = hits[::STEP]
        n = sel.size
        unit = rays[sel, 3:6] / np.linalg.norm(rays[sel, 3:6], axis=1, keepdims=True)
        pts = np.ascontiguousarray(rays[sel, 3:6] * frame["t"][sel, None] - unit * np.float32(OFF), np.float32)
        print(f"closest segments, K3 ground_bunny {W}x{H}: {g.flat.n_tris} triangles, {g.flat.n_nodes} nodes; every {STEP}th of {hits.size} hit points, {OFF} off the "
              f"surface: {n} segments; {rounds} rounds of {reps} calls, forms alternating; ms a call; min / max: the spread of the rounds")
        print(f"box test 2 compiled out: {'libsrt_hip_segments_no_box_test_2.so' if other else 'that build is not here, (c) is left out'}")
        print(f"{'segments':34s} {'form':34s} {'median':>8s} {'min':>8s} {'max':>8s} {'/ first':>7s}")
        tri, d2, s = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        d_pts = torch.from_numpy(pts).to(dev)

        def counts(o):
            st = o["stats"]
            return f"found {int((o['tri'] >= 0).sum())} of {n}; per item {st['node_tests_primary'] / n:.1f} node tests, {st['tri_tests_primary'] / n:.1f} triangle tests"
        # (a) the policy: point segments beside the point call
        seg0 = np.ascontiguousarray(np.concatenate([pts, pts], 1))
        d_seg0 = torch.from_numpy(seg0).to(dev)
        for r in (1.0, 4.0, 16.0):
            d_rad = torch.full((n,), r, dtype=torch.float32, device=dev)
            forms = {"closest_points (yardstick)": lambda: ds.closest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), stream=cur, tri=tri.data_ptr(), dist2=d2.data_ptr()),
                     "closest_segments, B = A": lambda: ds.closest_segments_device(n, d_seg0.data_ptr(), radius=d_rad.data_ptr(), stream=cur, tri=tri.data_ptr(), dist2=d2.data_ptr(),
                                                                                   s=s.data_ptr())}
            report(f"(a) points, radius {r:g}", rounds_of(forms, reps, rounds, side))
            side.synchronize()
            a, b = ds.closest_points(pts, radius=r, count=True, want=("tri", "dist2")), ds.closest_segments(seg0, radius=r, count=True, want=("tri", "dist2"))
            assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("tri", "dist2")) and a["stats"] == b["stats"]
            print(f"{'':34s} both: {counts(a)}")
        # (b), (c) segments of length L about the points
        rng = np.random.default_rng(9)
        u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        for L in (4.0, 32.0):
            seg = np.ascontiguousarray(np.concatenate([pts - u * (L / 2), pts + u * (L / 2)], 1), np.float32)
            d_seg = torch.from_numpy(seg).to(dev)
            for r in (1.0, 4.0):
                d_rad = torch.full((n,), r, dtype=torch.float32, device=dev)
                d_ball = torch.full((n,), r + L / 2, dtype=torch.float32, device=dev)
                forms = {f"closest_points, radius {r + L / 2:g}": lambda: ds.closest_points_device(n, d_pts.data_ptr(), radius=d_ball.data_ptr(), stream=cur, tri=tri.data_ptr(),
                                                                                                    dist2=d2.data_ptr()),
                         "closest_segments": lambda: ds.closest_segments_device(n, d_seg.data_ptr(), radius=d_rad.data_ptr(), stream=cur, tri=tri.data_ptr(), dist2=d2.data_ptr(),
                                                                                s=s.data_ptr())}
                if other:
                    forms["closest_segments, no box test 2"] = lambda: other.closest_segments_device(n, d_seg.data_ptr(), radius=d_rad.data_ptr(), stream=cur, tri=tri.data_ptr(),
                                                                                                       dist2=d2.data_ptr(), s=s.data_ptr())
                report(f"(b) length {L:g}, radius {r:g}", rounds_of(forms, reps, rounds, side))
                side.synchronize()
                ball, cap = ds.closest_points(pts, radius=r + L / 2, count=True, want=("tri", "dist2")), ds.closest_segments(seg, radius=r, count=True, want=("tri", "dist2", "feature"))
                print(f"{'':34s} the ball: {counts(ball)}")
                print(f"{'':34s} the segment: {counts(cap)}; crossings {int((cap['feature'][cap['tri'] >= 0] == 5).sum())}")
                if other:
                    wide = other.closest_segments(seg, radius=r, count=True, want=("tri", "dist2"))
                    same = all(np.array_equal(wide[k].view(np.uint32), cap[k].view(np.uint32)) for k in ("tri", "dist2"))
                    print(f"{'':34s} no box test 2: {counts(wide)}; same tri and dist2: {same}")
    if other:
        other.close()
    ds.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", action="store_true")
    ap.add_argument("--signed", action="store_true")
    ap.add_argument("--points", action="store_true")
    ap.add_argument("--points-multi", action="store_true", dest="points_multi")
    ap.add_argument("--nearest", action="store_true")
    ap.add_argument("--render-ao", action="store_true", dest="render_ao")
    ap.add_argument("--ao", action="store_true")
    ap.add_argument("--fresnel", action="store_true")
    ap.add_argument("--refract", action="store_true")
    ap.add_argument("--masked", action="store_true")
    ap.add_argument("--shadow-rule", action="store_true", dest="shadow_rule")
    ap.add_argument("--paths", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--shade", action="store_true")
    ap.add_argument("--range", action="store_true", dest="t_range")
    ap.add_argument("--shade-range", action="store_true", dest="shade_range")
    ap.add_argument("--multi", action="store_true")
    ap.add_argument("--surface", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    reps = 3 if a.trace else a.reps
    if a.segments:
        return segments_section(reps, 2 if a.trace else a.rounds)
    if a.signed:
        return signed_section(reps, 2 if a.trace else a.rounds)
    if a.points_multi:
        return points_multi_section(reps, 2 if a.trace else a.rounds)
    if a.points or a.nearest:
        return points_section(reps, 2 if a.trace else a.rounds, nearest=a.nearest)
    if a.render_ao:
        return render_ao_section(reps, 2 if a.trace else a.rounds)
    if a.ao:
        return ao_section(reps, 2 if a.trace else a.rounds)
    if a.fresnel:
        return fresnel_section(reps, 2 if a.trace else a.rounds)
    if a.refract:
        return refract_section(reps, 2 if a.trace else a.rounds)
    if a.masked:
        return masked_section(reps, 2 if a.trace else a.rounds)
    if a.shadow_rule:
        return shadow_rule_section(reps, 2 if a.trace else a.rounds)
    if a.paths:
        return paths_section(reps, 2 if a.trace else a.rounds)
    if a.multi:
        return multi_section(reps, 2 if a.trace else a.rounds)
    if a.surface:
        return surface_section(reps, 2 if a.trace else a.rounds)
    if a.shade:
        return shade_section(reps)
    if a.shade_range:
        return shade_range_section(reps, 2 if a.trace else a.rounds)
    if a.t_range:
        return range_section(reps, 2 if a.trace else a.rounds)
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    assert cur != 0
    print(f"K3 ground_bunny {W}x{H}: {g.flat.n_tris} triangles, {g.flat.n_nodes} nodes, {reps} repetitions each")
    # the yardsticks: ms_primary of the renders (HIP events inside the library, averaged over the renders since the last sync)
    ms = {}
    for name, flags in (("render, variant 2 (wave triangle queue)", 2 << 8), ("render, shipped pipeline", 0)):
        p = g.params(W, H, 1, flags=flags)
        for _ in range(2):
            ds.render(p, want=())
        for _ in range(reps):
            ds.render_device(p, stream=cur)
        st = ds.sync()
        ms[name] = st["ms_primary"]
        print(f"{name:44s} ms_primary {st['ms_primary']:8.3f}   ({ds.pipeline}, {st['launches']} launches)")
    yard = ms["render, variant 2 (wave triangle queue)"]
    rays = frame_rays()
    n = rays.shape[0]
    frame = ds.render(g.params(W, H, 1), want=("hit_id", "t"))
    hit_ref, t_ref = frame["hit_id"].reshape(-1), frame["t"].reshape(-1)
    orders = (("(a) tile order, 8x8 pixels a wave", tile_order()), ("(b) row-major", np.arange(n)), ("(c) randomly permuted", np.random.default_rng(1).permutation(n)))
    hit = torch.empty(n, dtype=torch.int32, device=dev); t = torch.empty(n, dtype=torch.float32, device=dev); bary = torch.empty((n, 3), dtype=torch.float32, device=dev)
    for name, order in orders:
        d_rays = torch.from_numpy(np.ascontiguousarray(rays[order])).to(dev)
        torch.cuda.synchronize()
        m1 = timed(lambda: ds.trace_rays_device(n, d_rays.data_ptr(), stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr()), reps, side)
        ok = np.array_equal(hit.cpu().numpy(), hit_ref[order]) and np.array_equal(t.cpu().numpy().view(np.uint32), t_ref[order].view(np.uint32))
        m2 = timed(lambda: ds.trace_rays_device(n, d_rays.data_ptr(), stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr(), bary=bary.data_ptr()), reps, side)
        print(f"query {name:38s} ms {m1:8.3f}   {n / m1 / 1e6:7.2f} Grays/s   x{m1 / yard:5.2f} of variant 2   with bary {m2:8.3f} ms   same bits as the frame: {ok}")
        assert ok
    # occlusion: the frame's shadow rays (so = d * t, sd = L - so), hit object skipped, in tile order and permuted
    sel = hit_ref >= 0
    L = np.asarray(g.light, np.float32).reshape(1, 3)
    so = rays[sel, 3:6] * t_ref[sel, None]
    sray = np.ascontiguousarray(np.concatenate([so, L - so], 1), np.float32)
    skip = g.flat.tri_obj[hit_ref[sel]].astype(np.int32)
    m = sray.shape[0]
    rank = np.empty(n, np.int64); rank[orders[0][1]] = np.arange(n)
    occ = torch.empty(m, dtype=torch.uint8, device=dev)
    for name, order in (("tile order", np.argsort(rank[sel], kind="stable")), ("randomly permuted", np.random.default_rng(2).permutation(m))):
        d_s = torch.from_numpy(np.ascontiguousarray(sray[order])).to(dev); d_k = torch.from_numpy(np.ascontiguousarray(skip[order])).to(dev)
        torch.cuda.synchronize()
        mo = timed(lambda: ds.occluded_device(m, d_s.data_ptr(), occ.data_ptr(), skip_obj=d_k.data_ptr(), stream=cur), reps, side)
        side.synchronize()
        print(f"occlusion, {m} shadow rays, {name:18s} ms {mo:8.3f}   {m / mo / 1e6:7.2f} Grays/s   occluded {int(occ.sum().item())}")
    # host entry point, end to end (staging, copies, wait)
    for k in (1, n):
        r = np.ascontiguousarray(rays[orders[0][1]][:k])
        ds.trace_rays(r); ds.trace_rays(r)
        t0 = time.perf_counter()
        for _ in range(reps):
            ds.trace_rays(r)
        full = (time.perf_counter() - t0) / reps * 1e3
        t0 = time.perf_counter()
        for _ in range(reps):
            ds.trace_rays(r, want=())
        print(f"srt_trace_rays end to end, {k:8d} rays: {full:9.3f} ms a call (hit_id, t, bary to host arrays); without the copies back {(time.perf_counter() - t0) / reps * 1e3:9.3f} ms")


if __name__ == "__main__":
    main()
