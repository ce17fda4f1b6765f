"""SamAutomaticMaskGenerator timing at 1080p with default parameters (32x32 points, 64 per batch, 3 masks each) on synthetic
weights: a ViT-B-sized SAM encoder and a Hiera-B+ encoder, each with the exact and the f16 decoder plan.  Device events around
generate() and around each stage run alone with the same shapes: encoder (set_image), the 16 decoder batches
(decode_lowres of 64 prompts), the 16 lmx_k_mask_score launches (192 candidates each, 1080x1920) and lmx_k_nms_boxes over 3 072
candidates.  Prints one JSON line per configuration.

  python tools/amg_probe.py [--reps 3] [--models vit_b,hiera_bp] [--plans exact,f16]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-sam3-yolo-lameless_amd")]

from lmx import adapters, sam, sam_decoder, synth, weights  # noqa: E402
from lmx import kernels as K  # noqa: E402


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def predictor(name, dev):
    dsd = sam_decoder.synthetic_state_dict(62)
    if name == "vit_b":
        cfg = sam.SamVitConfig(hidden=768, layers=12, heads=12, mlp=3072, global_idx=(2, 5, 8, 11), window=14, image=1024)
        sd = weights.synth_state_dict(sam.vit_param_spec(cfg), 61)
        sd.update(dsd)
        return adapters.SamPredictor(adapters.LmxSam(cfg, sd, dev))
    cfg = sam.hiera_b_plus()
    enc = sam.HieraEncoder(cfg, weights.synth_state_dict(sam.param_spec(cfg), 11), dev)
    return adapters.LmxSamPredictor.from_parts(enc, sam_decoder.MaskDecoder(dsd, dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--models", default="vit_b,hiera_bp")
    ap.add_argument("--plans", default="exact,f16")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    image = synth.synth_frame(6, 20)[..., ::-1].copy()  # 1080x1920 RGB
    for name in args.models.split(","):
        pred = predictor(name, dev)
        for plan in args.plans.split(","):
            pred.decoder.precision = plan
            gen = adapters.SamAutomaticMaskGenerator(pred)
            recs = gen.generate(image)  # warm-up (and the record count)
            t_gen = timed(lambda: gen.generate(image), args.reps)
            t_enc = timed(lambda: pred.set_image(image), args.reps)
            H, W = pred.original_size
            nh, nw = pred.input_size
            pts = gen.point_grids[0] * np.array([[W, H]])
            tp = torch.from_numpy(pred.transform.apply_coords(pts, (H, W)).astype(np.float32)).to(dev)[:, None].contiguous()
            lab = torch.ones((len(pts), 1), dtype=torch.int32, device=dev)
            lows = []

            def dec():
                lows.clear()
                for b0 in range(0, len(pts), 64):
                    lr, _ = pred.decoder.decode_lowres(pred.features, (H, W), (nh, nw), points=tp[b0:b0 + 64], labels=lab[b0:b0 + 64],
                                                       multimask=True, input_frame=True)
                    lows.append(lr.view(-1, 256, 256))

            t_dec = timed(dec, args.reps)
            t_score = timed(lambda: [K.mask_score(lr, pred.decoder.S, nh, nw, H, W, 0.0, 1.0) for lr in lows], args.reps)
            st = torch.cat([K.mask_score(lr, pred.decoder.S, nh, nw, H, W, 0.0, 1.0) for lr in lows])
            iou = torch.rand(st.shape[0], device=dev)
            t_nms = timed(lambda: K.nms_boxes(st[:, 3:7].float(), iou, 0.7), args.reps)
            px = st.shape[0] * H * W
            print(json.dumps(dict(model=name, plan=plan, frame=[H, W], candidates=int(st.shape[0]), records=len(recs),
                                  generate_ms=round(t_gen, 2), encoder_ms=round(t_enc, 2), decoder_ms=round(t_dec, 2),
                                  mask_score_ms=round(t_score, 3), nms_ms=round(t_nms, 3),
                                  mask_score_gpix_per_s=round(px / t_score / 1e6, 1))), flush=True)


if __name__ == "__main__":
    main()
