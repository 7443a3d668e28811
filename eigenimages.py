#!/usr/bin/env python3
"""How the members of a class differ from their average: per class of aligned images, the variance map and the leading
eigenimages of the covariance about the class average (multivariate statistical analysis; eigen-galaxies for the galaxy
script), with every image's coordinates along them.  Reads the model as infer.py does, the poses from the score file infer.py
wrote for the same model and split, and optionally a label file; walks the split on the device and writes one .npz.  The
reference has no such entry point.  The work is in spatial_vae_amd/eigen_images.py (eigen_main) and ops.EigenImages.

  python infer.py mnist --state run_state_epoch10.ckpt --out scores.npz
  python eigenimages.py mnist --state run_state_epoch10.ckpt --scores scores.npz --labels l.npy --out eigen.npz
  python eigenimages.py particles --state run_state_epoch20.ckpt --scores s.npz --pose refined --components 4 --out eigen.npz
"""
import importlib
import sys

from infer import TRAINERS


def main(argv=None):
    from spatial_vae_amd import eigen_images as pipeline
    args = pipeline.eigen_arguments(argv)
    module, parser, positional = TRAINERS[args.script]
    trainer = importlib.import_module(module)
    return pipeline.eigen_main(args, getattr(trainer, parser), trainer.build, positional)


if __name__ == "__main__":
    sys.exit(main())
