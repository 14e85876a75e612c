"""vtp_amd -- MI355X-native (gfx950 / CDNA4) VTP training hot path.

Public surface mirrors the reference (`from vtp.models.vtp_hf import VTPConfig, VTPModel`):
    from vtp_amd import VTPConfig, VTPModel, VTPTrainer, LinearProbe, ZeroShot, Knn, ReconEval, MultiCrop, Preprocess, FID,
    InceptionFeatures, FrechetStats, frechet_distance, PrecisionRecall, InceptionScore, GenEval, Retrieval, KID, SegProbe,
    DepthProbe
Everything below the Python API is hand-written HIP in libvtp_hip.so (C ABI: include/vtp_hip.h)."""
from .config import VTPConfig  # noqa: F401


def __getattr__(name):  # lazy: importing the package must not require torch.cuda
    if name == "VTPModel":
        from .model import VTPModel
        return VTPModel
    if name == "VTP":
        from .vtp import VTP
        return VTP
    if name == "LPIPS":
        from .lpips import LPIPS
        return LPIPS
    if name == "VTP_Tokenizer":
        from .tokenizer import VTP_Tokenizer
        return VTP_Tokenizer
    if name == "patch_model":
        from .patch import patch_model
        return patch_model
    if name == "VTPTrainer":
        from .train import VTPTrainer
        return VTPTrainer
    if name == "LinearProbe":
        from .probe import LinearProbe
        return LinearProbe
    if name == "SegProbe":
        from .segprobe import SegProbe
        return SegProbe
    if name == "DepthProbe":
        from .depthprobe import DepthProbe
        return DepthProbe
    if name == "ZeroShot":
        from .zeroshot import ZeroShot
        return ZeroShot
    if name == "Knn":
        from .knn import Knn
        return Knn
    if name == "ReconEval":
        from .recon_eval import ReconEval
        return ReconEval
    if name == "MultiCrop":
        from .augment import MultiCrop
        return MultiCrop
    if name == "Preprocess":
        from .preprocess import Preprocess
        return Preprocess
    if name in ("InceptionFeatures", "FrechetStats", "FID", "frechet_distance"):
        from . import fid
        return getattr(fid, name)
    if name == "PrecisionRecall":
        from .precision_recall import PrecisionRecall
        return PrecisionRecall
    if name in ("InceptionScore", "inception_score_from_sums"):
        from . import inception_score
        return getattr(inception_score, name)
    if name == "GenEval":
        from .gen_eval import GenEval
        return GenEval
    if name == "Retrieval":
        from .retrieval import Retrieval
        return Retrieval
    if name == "KID":
        from .kid import KID
        return KID
    raise AttributeError(name)
