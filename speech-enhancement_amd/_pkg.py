"""MI355X-native CMGAN / SCP-GAN hot path.  Public surface = the reference's Python call surface
for this path."""
from . import _lib  # noqa: F401
from .generator import TSCNet  # noqa: F401
from .discriminator import Discriminator, LearnableSigmoid, batch_pesq  # noqa: F401
from .frontend import compressed_stft, uncompressed_istft, normalize_batch  # noqa: F401
from .train import train_gan, validate_gan, batch_stft, gan_step, set_pesq_provider  # noqa: F401
from .optim import build_optimizer, set_weight_decay, LARS, Lamb  # noqa: F401
from .utils import adjust_learning_rate, kaiming_init, save_checkpoint  # noqa: F401
from .config import get_config  # noqa: F401
from .inference import load_model, predict  # noqa: F401
from .criterion import build_criterion  # noqa: F401
from .frontend import disassemble_spectrogram, power_compress, power_uncompress  # noqa: F401
from .diffuse import DiffuSE, inference_schedule  # noqa: F401
from .diffuse import predict as predict_diffuse  # noqa: F401
from .tsc_diffusion import TSCNetDiffusion, predict_tsc, tsc_diffusion_step, tsc_diffusion_validation_loss, add_noise  # noqa: F401
from .train import set_pesq_score_provider  # noqa: F401
from .metrics import compute_metrics, evaluate  # noqa: F401
from .data import DeviceDataset, DeviceLoader, read_wav, resample  # noqa: F401
from .data import NoiseBank, BankMix, bank_rng, draw_bank, mix_bank_at_snr  # noqa: F401
from .sampler import GraphedTSCSampler, sampler_update, philox_normal  # noqa: F401
from .tsc_diffusion import noise_coefficients, draw_steps, diffusion_noise, pack_counter  # noqa: F401
from .train_diffuse import train_tsc_diffusion, validate_tsc_diffusion  # noqa: F401
from .inference import LongEnhancer, chunk_plan  # noqa: F401
from .inference import StreamEnhancer, check_streaming  # noqa: F401
