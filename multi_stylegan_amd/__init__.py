"""Multi-StyleGAN generator + discriminator training hot path, MI355X-native (gfx950 HIP kernels behind the
reference's nn.Module / op_static API).  See DESIGN.md.  Public names follow multi_stylegan/__init__.py."""
from .adaptive_discriminator_augmentation import AdaptiveDiscriminatorAugmentation, AugmentationPipeline
from .config import (generation_hyperparameters, multi_style_gan_generator_config,
                     u_net_2d_discriminator_config)
from .data import DevicePrefetcher, SyntheticBatches, TLFMDeviceFeed, prepare_tlfm_batch
from .elastic import ElasticDeformation, elastic_deform_batch, elastic_deformation
from .inference import GeneratorSampler, load_generator_ema, split_sequences, validation_samples
from .loss import (HingeDiscriminatorLoss, HingeDiscriminatorLossCutMix, HingeGeneratorLoss, PathLengthRegularization,
                   R2Regularization, TopK, WassersteinDiscriminatorLoss, WassersteinDiscriminatorLossCutMix,
                   WassersteinGeneratorLoss)
from .model_wrapper import Draws, ModelWrapper
from .multi_stylegan_generator import Generator as MultiStyleGANGenerator
from .resident import ResidentTLFMFeed, ResidentTLFMStore, gather_tlfm_batch
from .u_net_2d_discriminator import Discriminator as MultiStyleGANDiscriminator
from .samples import (SheetWriter, dump_samples, epoch_sample_dump, interpolation_frames, interpolation_latents, sample_sheets,
                      save_prediction, write_png)
from .simulate import (TLFMDatasetWriter, bf_ranges_like, export_tlfm_batch, simulate_dataset, simulation_latents, write_tiff)
from .tlfm_dataset import TFLMDatasetGAN, read_tiff
from .validation_metrics import (FID, FVD, IS, KID, KVD, FeatureRows, ManifoldScores, PrecisionRecall, PrecisionRecallVideo,
                                 kernel_distance, manifold_scores, metric_inputs, SWD, SWVD, laplacian_pyramid,
                                 sliced_wasserstein, MSSSIM, MSSSIMVideo, DiversityScore)
from .ssim import MS_SSIM_WEIGHTS, ms_ssim, ssim_levels
from .project import Projection, mean_latent, project_sequences, truncate
from .video import MjpegWriter, interpolation_video, jpeg_encode, jpeg_file, jpeg_tables

__all__ = ["MultiStyleGANGenerator", "MultiStyleGANDiscriminator", "ModelWrapper", "Draws", "PathLengthRegularization",
           "TopK", "AdaptiveDiscriminatorAugmentation", "AugmentationPipeline", "GeneratorSampler", "load_generator_ema", "split_sequences", "validation_samples",
           "DevicePrefetcher", "SyntheticBatches", "TLFMDeviceFeed", "prepare_tlfm_batch", "TFLMDatasetGAN", "read_tiff",
           "sample_sheets", "write_png", "SheetWriter", "save_prediction", "epoch_sample_dump", "dump_samples", "interpolation_latents",
           "interpolation_frames", "IS", "FID", "FVD", "metric_inputs", "multi_style_gan_generator_config", "u_net_2d_discriminator_config", "generation_hyperparameters",
           "WassersteinDiscriminatorLoss", "WassersteinDiscriminatorLossCutMix", "WassersteinGeneratorLoss", "HingeGeneratorLoss",
           "HingeDiscriminatorLoss", "HingeDiscriminatorLossCutMix", "R2Regularization", "ElasticDeformation", "elastic_deformation",
           "elastic_deform_batch", "ResidentTLFMStore", "ResidentTLFMFeed", "gather_tlfm_batch", "jpeg_tables", "jpeg_encode", "jpeg_file",
           "MjpegWriter", "interpolation_video", "export_tlfm_batch", "write_tiff", "TLFMDatasetWriter", "bf_ranges_like",
           "simulate_dataset", "simulation_latents", "KID", "KVD", "PrecisionRecall", "PrecisionRecallVideo", "FeatureRows",
           "ManifoldScores", "kernel_distance", "manifold_scores", "SWD", "SWVD", "laplacian_pyramid", "sliced_wasserstein",
           "MSSSIM", "MSSSIMVideo", "DiversityScore", "ms_ssim", "ssim_levels", "MS_SSIM_WEIGHTS", "Projection", "mean_latent",
           "project_sequences", "truncate"]
