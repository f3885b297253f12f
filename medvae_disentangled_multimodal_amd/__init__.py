"""MI355X-native conv-VAE training hot path (drop-in for parsakzr/medvae-disentangled-multimodal's
src.models / src.losses / VAELightningModule on the training step)."""
from .disentangled import DisentangledConditionalVAE
from .encoder_decoder import (AttnBlock, Decoder, Downsample, Encoder, LinAttnBlock, LinearAttention, ResnetBlock,
                              Upsample)
from .evaluation import evaluate_model
from .lightning_module import VAELightningModule
from .losses import DisentangledVAELoss, LPIPSLoss, LPIPSWithDiscriminator, VAELoss
from .lpips import LPIPS
from .metrics import (compute_kl_metrics, compute_kl_metrics_device, compute_latent_metrics,
                      compute_latent_metrics_device, compute_reconstruction_metrics,
                      compute_reconstruction_metrics_device)
from .optim import Adam, AdamW, FlatParameters, FusedAdam
from .schedulers import get_scheduler
from .vae import BaseVAE, BetaVAE, ConditionalVAE

__all__ = ["BaseVAE", "BetaVAE", "ConditionalVAE", "DisentangledConditionalVAE", "DisentangledVAELoss",
           "VAELoss", "LPIPSLoss", "LPIPSWithDiscriminator", "LPIPS", "Encoder", "Decoder", "ResnetBlock", "AttnBlock",
           "LinearAttention", "LinAttnBlock", "Downsample", "Upsample",
           "VAELightningModule", "FlatParameters", "FusedAdam", "Adam", "AdamW", "get_scheduler", "evaluate_model",
           "compute_reconstruction_metrics", "compute_reconstruction_metrics_device", "compute_kl_metrics",
           "compute_kl_metrics_device", "compute_latent_metrics", "compute_latent_metrics_device"]
