"""The tiled decode of a wide latent beside the plain decode of the same windows, on the MI355X (profiles/windowed_latent.md).

    python tools/windowed_latent_probe.py [--trace]

The config-4 VAE (config/ldm_autoencoder_kl.yaml: 256x256 image, block_out_channels 128-256-512-512, two layers per block, f = 8, a
32x32 latent) with random weights, B = 4 wide latents, stride W/2 = 16 latent columns, open placement, `frames` = 4x and 8x the model
width. Device events around each synchronised call; one warm-up call per shape first (plan, first launches); PROBE_RUNS (default 5)
timed calls each, the two decodes alternating. One JSON line per measurement:

  decode   `decode_tiled(z, 32, 16, _in_scale=1/0.18215, want_u8=True)` on (4, 1, 32, frames), against `decode` of a (4*nW, 1, 32, 32)
           latent batch (what the decoder itself costs at that batch; the difference is gather + cross-fade)
  kernel   `ops.window_crossfade(..., want_u8=True)` alone on the decoded windows, PROBE_LAUNCHES (default 50) launches back to back
           between two events, and the bytes of its traffic formula (4 B read per window element + 5 B written per wide element) over
           that time. The windows of one call (up to 15.7 MB per sample row) do not all stay in a cache between launches at these sizes,
           but the figure is a rate over back-to-back launches from Python (each pays its enqueue), not a trace's kernel time.
--trace:  one warm-up and three `decode_tiled` calls per width and nothing else, for a kernel trace taken from outside: the kernel time of
          `window_crossfade_kernel` and `window_gather_kernel`, over which the traffic formula gives the achieved bytes/s."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS, LAUNCHES = int(os.environ.get("PROBE_RUNS", "5")), int(os.environ.get("PROBE_LAUNCHES", "50"))
VAE = dict(sample_size=(256, 256), in_channels=1, out_channels=1, latent_channels=1, layers_per_block=2,
           block_out_channels=(128, 256, 512, 512), down_block_types=("DownEncoderBlock2D",) * 4, up_block_types=("UpDecoderBlock2D",) * 4)
B, W, STRIDE, F = 4, 32, 16, 8


def timed(dev, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return round(a.elapsed_time(b), 3)


def main(dev, trace):
    from audiodiffusion import AutoencoderKL, ops
    vae = AutoencoderKL(**VAE).init_random(0)
    g = torch.Generator().manual_seed(8)
    for mult in (4, 8):
        frames = mult * W
        nW = ops.window_count(frames, W, STRIDE, False)
        z = (0.18215 * torch.randn(B, 1, W, frames, generator=g)).to(dev)
        zb = ops.window_gather(z, W, STRIDE, False)
        tiled = lambda: vae.decode_tiled(z, W, STRIDE, False, _in_scale=1 / 0.18215, want_u8=True)   # noqa: E731
        plain = lambda: vae.decode(zb, _in_scale=1 / 0.18215)                                        # noqa: E731
        tiled(), plain()
        if trace:
            print(json.dumps(dict(what="trace", frames=frames, crossfade_traffic_bytes=4 * zb.shape[0] * F * W * F * W + 5 * B * F * W * F * frames,
                                  decode_tiled_ms=[timed(dev, tiled) for _ in range(3)])), flush=True)
            continue
        tt, tp = [], []
        for _ in range(RUNS):
            tt.append(timed(dev, tiled))
            tp.append(timed(dev, plain))
        print(json.dumps(dict(what="decode", frames=frames, windows_per_sample=nW, decoder_batch=B * nW, decode_tiled_ms=tt,
                              plain_decode_ms=tp, difference_ms=[round(a - b, 3) for a, b in zip(tt, tp)])), flush=True)
        pixels = plain()["sample"]
        fade = lambda: ops.window_crossfade(pixels, F * frames, F * STRIDE, False, want_u8=True)     # noqa: E731
        fade()

        def many():
            for _ in range(LAUNCHES):
                fade()
        traffic = 4 * pixels.numel() + 5 * B * F * W * F * frames
        tk = [round(timed(dev, many) / LAUNCHES, 4) for _ in range(RUNS)]
        print(json.dumps(dict(what="kernel", frames=frames, traffic_bytes=traffic, crossfade_ms_per_launch=tk,
                              achieved_GBps=[round(traffic / (t * 1e-3) / 1e9, 1) for t in tk])), flush=True)
        del pixels, z, zb
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "audio-diffusion_amd"), ROOT]
    assert torch.cuda.is_available(), "this probe times the MI355X: no GPU, no number"
    main(torch.device("cuda:0"), args.trace)
