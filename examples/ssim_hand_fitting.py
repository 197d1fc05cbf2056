"""The colour fit of the hand (examples/rgb_image_hand_fitting.py) against a photograph whose intensities were scaled and offset -- an exposure the
lighting model does not explain --, with the plain L2 data term and with the structural one mixed in (``ssim_weight=``, deodr_amd/ssim.py): the
pixel term pays for the exposure with the colour and the lights and keeps pulling on the geometry, ``1 - SSIM`` under its 11 x 11 Gaussian window
compares local means, contrasts and correlations and moves far less.

    python examples/ssim_hand_fitting.py [--iterations 200] [--ssim-weight 0.2] [--gain 0.7] [--offset 0.1] [--eager]

Prints both energy curves (each in its own data term) and, for comparison, both data terms of both fits against the photograph AS IT WAS at the end.
"""
import argparse

import numpy as np

from _common import golden, hand_mesh, run


def make_fitter(image, **keywords):
    from deodr_amd.mesh_fitter import MeshRGBFitterWithPose

    r = golden("rgb_hand_fit.npz")  # hand.png of the reference, the constants of its example
    _vertices, faces = hand_mesh()
    fitter = MeshRGBFitterWithPose(r["vertices_centered"], faces, np.zeros(3), r["translation_init"], r["default_color"], r["default_light_directional"],
                                   float(r["default_light_ambient"]), cregu=1000, **keywords)  # fmt: skip
    fitter.set_image(image)
    fitter.set_background_color(r["background_color"])
    return fitter


def main(iterations=200, ssim_weight=0.2, gain=0.7, offset=0.1, graph=True):
    import torch

    from deodr_amd.mesh_fitter import GraphedStep
    from deodr_amd.ssim import ssim_terms

    photograph = golden("rgb_hand_fit.npz")["image_u8"].astype(np.float64) / 255
    exposed = np.clip(gain * photograph + offset, 0, 1)
    curves, fitters = [], []
    for label, keywords in (("plain L2", {}), (f"ssim_weight = {ssim_weight}", dict(ssim_weight=ssim_weight))):
        fitter = make_fitter(exposed, **keywords)
        stepper = GraphedStep(fitter) if graph else fitter
        curves.append(run(lambda: stepper.step_device()[0], iterations, max(iterations // 10, 1), label))
        fitters.append((label, fitter))
    target = torch.as_tensor(photograph, device=fitters[0][1].device)[None]
    for label, fitter in fitters:
        t0, t1 = ssim_terms(fitter.render(), target).tolist()
        print(f"{label}: against the photograph as it was, after {iterations} iterations: squared residual {t0:.3f}, sum of 1 - SSIM {t1:.3f}")
    return curves


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--ssim-weight", type=float, default=0.2)
    ap.add_argument("--gain", type=float, default=0.7)
    ap.add_argument("--offset", type=float, default=0.1)
    ap.add_argument("--eager", action="store_true", help="launch the kernels of every iteration from the host instead of replaying a HIP graph")
    a = ap.parse_args()
    main(a.iterations, a.ssim_weight, a.gain, a.offset, not a.eager)
