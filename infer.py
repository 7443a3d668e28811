#!/usr/bin/env python3
"""Apply a trained spatial-VAE to a dataset: per image, the inferred rotation and translation, the content latents and the
K-sample importance-weighted bound on log p(x), streamed in chunks so that K is not limited by memory.  One .npz, one row per
image in dataset order.  On request also what the poses are for: every image brought into the model's canonical frame
(--aligned), its pose-free reconstruction (--recon) and the averages of the aligned images, overall or per class of --labels
(--class_averages); for particles with a CTF table, --ctf_correct flip / wiener corrects each image by its own transfer function
first.  The reference has no such entry point (its command lines end at the .sav files and the table of
minibatch means).  The work is in spatial_vae_amd/infer.py (infer_main) and spatial_vae_amd/elbo.py (score_minibatch,
align_minibatch, reconstruct_unposed).

  python infer.py mnist --state outputs_run/trained/run_state_epoch10.ckpt --out scores.npz --num_samples 5000 --chunk 50
  python infer.py particles --generator G.sav --inference Q.sav --out s.npz -- train.mrcs test.mrcs --z-dim 4 --mask
  python infer.py particles --state run_state_epoch20.ckpt --out s.npz --aligned aligned.mrcs --class_averages classes.npz --labels l.npy
  python infer.py particles --state run_state_epoch20.ckpt --out s.npz --ctf_correct wiener --class_averages classes.npz --labels l.npy
"""
import importlib
import sys

# script -> (module, its argument function, stand-ins for its positional arguments)
TRAINERS = {"mnist": ("train_mnist", "mnist_arguments", ()),
            "galaxy": ("train_galaxy", "galaxy_arguments", ("train.npy", "test.npy")),
            "particles": ("train_particles", "particle_arguments", ("train.mrcs", "test.mrcs"))}


def main(argv=None):
    from spatial_vae_amd import infer as pipeline
    args = pipeline.infer_arguments(argv)
    module, parser, positional = TRAINERS[args.script]
    trainer = importlib.import_module(module)
    return pipeline.infer_main(args, getattr(trainer, parser), trainer.build, positional)


if __name__ == "__main__":
    sys.exit(main())
