"""fplx - MI355X-native hot path of FPL+ (3D U-Net with domain-specific BatchNorm, segmentation
losses, pseudo-label uncertainty filter) behind PyMIC's registry / agent surface.

Everything numeric runs in hand-written HIP kernels (libfplx.so, C ABI in include/fplx.h);
importing the package without the built library raises - there is no CPU fallback.
"""
from . import _lib

_lib.lib()          # fail loudly, now, if the HIP extension is missing

from .net import UNet2D5_dsbn                                      # noqa: E402
from .nets3d import UNet2D5, UNet3D                                # noqa: E402
from .dsbn import DomainSpecificBatchNorm3d                        # noqa: E402
from .loss import (SegLossDict, DiceLoss, CrossEntropyLoss, DiceLoss_weight, CombinedLoss,  # noqa: E402
                   EntropyTerm, make_loss, SegLossDictAll, FocalDiceLoss, NoiseRobustDiceLoss, ExpLogLoss,
                   GeneralizedCELoss, MAELoss, MSELoss, SLSRLoss, DeepSuperviseLoss)
from .infer import Inferer                                         # noqa: E402
from .agent import SegmentationAgent, SegNetDict                   # noqa: E402
from .optim import (FusedOptimizer, FusedAdam, FusedSGD, FusedAdadelta, FusedAdagrad, FusedAdamax, FusedASGD,  # noqa: E402
                    FusedRMSprop, FusedRprop, get_optimizer, get_lr_scheduler)
from .train import TrainStep                                       # noqa: E402
from .config import parse_config, synchronize_config               # noqa: E402
from .dataset import NiftyDataset                                  # noqa: E402
from .postprocess import PostProcess, PostKeepLargestComponent, PostProcessDict, get_largest_k_components  # noqa: E402
from .ssl import (SSLSegAgent, SSLEntropyMinimization, SSLMeanTeacher, SSLUncertaintyAwareMeanTeacher,   # noqa: E402
                  SSLMethodDict, EntropyLoss, consistency_loss, ema_update, get_rampup_ratio,
                  SSLCPS, SSLURPC, SSLMethodDictAll, ssl_agent_class_all, pyramid_consistency_loss, cross_pseudo_labels)
from .wsl import (WSLSegAgent, WSLEntropyMinimization, WSLTotalVariation, WSLMumfordShah, WSLGatedCRF, WSLUSTM,  # noqa: E402
                  WSLMethodDict, TotalVariationLoss, MumfordShahLoss, GatedCRFLoss)
from .nll import (NLLSegAgent, NLLCoTeaching, NLLTriNet, NLLMethodDict, nll_agent_class, BiNet, TriNet,          # noqa: E402
                  GroupOptimizer, selective_ce_loss)
from .image_process import distance_transform_edt, get_euclidean_distance                                   # noqa: E402
from .confident import (get_confident_map, get_noise_indices, compute_confident_joint, calibrate_confident_joint,   # noqa: E402
                        keep_at_least_n_per_class, round_preserving_sum)
from .nll_clslsr import NLLCLSLSR, get_confidence_map                                                        # noqa: E402
from . import confident, nll_clslsr                                                                          # noqa: E402
from . import filter, ops, ddp, transform, nifti, evaluation, postprocess, ssl, wsl, nll, netgroup, resample, image_process   # noqa: E402

__all__ = ["UNet2D5_dsbn", "DomainSpecificBatchNorm3d", "SegLossDict", "SegNetDict", "DiceLoss",
           "CrossEntropyLoss", "DiceLoss_weight", "CombinedLoss", "EntropyTerm", "make_loss", "Inferer",
           "SegmentationAgent", "FusedOptimizer", "FusedAdam", "FusedSGD", "FusedAdadelta", "FusedAdagrad", "FusedAdamax", "FusedASGD",
           "FusedRMSprop", "FusedRprop", "get_optimizer", "get_lr_scheduler", "TrainStep",
           "parse_config", "synchronize_config", "filter", "ops", "ddp", "transform", "nifti", "evaluation", "NiftyDataset",
           "postprocess", "SegLossDictAll", "FocalDiceLoss", "NoiseRobustDiceLoss", "ExpLogLoss", "GeneralizedCELoss", "MAELoss",
           "MSELoss", "SLSRLoss", "DeepSuperviseLoss", "UNet2D5", "UNet3D", "PostProcess", "PostKeepLargestComponent", "PostProcessDict", "get_largest_k_components",
           "ssl", "SSLSegAgent", "SSLEntropyMinimization", "SSLMeanTeacher", "SSLUncertaintyAwareMeanTeacher", "SSLMethodDict",
           "EntropyLoss", "consistency_loss", "ema_update", "get_rampup_ratio",
           "SSLCPS", "SSLURPC", "SSLMethodDictAll", "ssl_agent_class_all", "pyramid_consistency_loss", "cross_pseudo_labels",
           "netgroup",
           "wsl", "WSLSegAgent", "WSLEntropyMinimization", "WSLTotalVariation", "WSLMumfordShah", "WSLGatedCRF", "WSLUSTM",
           "WSLMethodDict", "TotalVariationLoss", "MumfordShahLoss", "GatedCRFLoss",
           "nll", "NLLSegAgent", "NLLCoTeaching", "NLLTriNet", "NLLMethodDict", "nll_agent_class", "BiNet", "TriNet",
           "GroupOptimizer", "selective_ce_loss",
           "resample", "image_process", "distance_transform_edt", "get_euclidean_distance",
           "confident", "nll_clslsr", "get_confident_map", "get_noise_indices", "compute_confident_joint",
           "calibrate_confident_joint", "keep_at_least_n_per_class", "round_preserving_sum", "NLLCLSLSR", "get_confidence_map"]
