#!/usr/bin/env python3
"""One denoised image per image, without choosing classes: for every image of a split its K nearest neighbours among the content
latents infer.py stored (exact, under the order (squared distance, image index)), the graph's statistics (found, in_degree), and
with --averages the average of the image and its neighbours, each aligned at its stored pose.  Reads the model as infer.py does
and the score file infer.py wrote for the same model and split; works on the device and writes one .npz.  The reference has no
such entry point.  The work is in spatial_vae_amd/neighbours.py (neighbour_main), ops.NeighbourSearch and ops.neighbour_average.

  python infer.py mnist --state run_state_epoch10.ckpt --out scores.npz
  python neighbours.py mnist --state run_state_epoch10.ckpt --scores scores.npz --out nbr.npz --averages avg.npy
  python neighbours.py particles --state run_state_epoch20.ckpt --scores s.npz --pose refined --neighbours 64 --weights gaussian \
      --out nbr.npz --averages avg.mrcs
"""
import importlib
import sys

from infer import TRAINERS


def main(argv=None):
    from spatial_vae_amd import neighbours as pipeline
    args = pipeline.neighbour_arguments(argv)
    module, parser, positional = TRAINERS[args.script]
    trainer = importlib.import_module(module)
    return pipeline.neighbour_main(args, getattr(trainer, parser), trainer.build, positional)


if __name__ == "__main__":
    sys.exit(main())
