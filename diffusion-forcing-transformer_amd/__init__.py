"""MI355X-native DFoT denoising engine (hot path only): HIP kernels behind a C ABI
(``csrc/`` -> ``libdfot_hip.so``, ``include/dfot_hip.h``) plus the host-side mirror of the
reference's backbone / sampler interfaces.  Importing it requires the built HIP library --
there is no CPU fallback."""
from . import capi  # noqa: F401  (raises ImportError when libdfot_hip.so is missing)
from . import ops  # noqa: F401  (registers the torch.library operators dfot::*)
from .ops import frame_causal_attention  # noqa: F401  (differentiable drop-in for SDPA under the block-lower-triangular mask)
from .ops import attention_seq64  # noqa: F401  (differentiable drop-in for SDPA over 64-token sequences: the per-frame attention at res-128)
from .backbone import UViT3DPose  # noqa: F401
from .uvit3d_backbone import UViT3D  # noqa: F401
from .dit_backbone import DiT3D, DifferenceDiT3D  # noqa: F401
from .dit1d_backbone import DiT1D  # noqa: F401
from . import attention_maps  # noqa: F401
from .attention_maps import frame_map, to_hook_layout  # noqa: F401
from .diffusion import DiffusionConfig, Schedule  # noqa: F401
from .guidance import HistoryGuidance  # noqa: F401
from .sampler import (DFoTVideoPoseSampler, DFoTVideoSampler, DifferenceDFoTVideoSampler, SamplerConfig,  # noqa: F401
                      device_noise_fn)  # noqa: F401
from . import parallel  # noqa: F401,E402
from .training import ContextTraining, TrainingNoise, training_step_forward  # noqa: F401,E402
from .checkpoint import load_reference_checkpoint  # noqa: F401,E402
from .trainer import DiT3DTrainer, FacDiTTrainer, FacMatDiTTrainer  # noqa: F401,E402
from .dit1d_trainer import DiT1DTrainer  # noqa: F401,E402
from . import uvit_train  # noqa: F401,E402
from .uvit_train import UViT3DPoseTrainer, UViT3DTrainer  # noqa: F401,E402
from .vae import VideoVAEDecoder, VideoVAEEncoder, VideoVAEPosterior, decode_latents, encode_videos  # noqa: F401,E402
from .image_vae import (ImageVAEDecoder, ImageVAEEncoder, ImageVAEPosterior, decode_image_latents,  # noqa: F401,E402
                        encode_image_frames, ddconfig_from_diffusers, diffusers_to_reference_keys,  # noqa: F401,E402
                        load_diffusers_checkpoint)  # noqa: F401,E402
from .titok import (TiTokDecoder, TiTokEncoder, decode_titok_latents, encode_titok_frames,  # noqa: F401,E402
                    load_titok_checkpoint)  # noqa: F401,E402
from .dcae import (DCAEDecoder, DCAEEncoder, dcae_config, decode_dcae_latents, encode_dcae_frames,  # noqa: F401,E402
                   load_dcae_checkpoint)  # noqa: F401,E402
