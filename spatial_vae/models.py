"""Drop-in for the reference's ``spatial_vae.models`` (same import path, same classes):
``import spatial_vae.models as models`` keeps working; the classes are defined in spatial_vae_amd.models and carry THIS
module's name as their class path, so whole-module pickles (torch.save(net)) interchange with the reference's."""
from spatial_vae_amd.models import InferenceNetwork, ResidLinear, SpatialGenerator, VanillaGenerator  # noqa: F401
