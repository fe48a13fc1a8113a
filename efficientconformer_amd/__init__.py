"""efficientconformer_amd — MI355X (gfx950) native Efficient Conformer encoder forward path.

Host-side mirror of the reference's encoder interface (models/encoders.ConformerEncoder,
models/model_ctc.ModelCTC) over the C ABI of include/effconf.h; the compute is hand-written HIP in
csrc/.  See DESIGN.md / INTEGRATION.md.
"""
from .config import build_plan, load_config, named_config  # noqa: F401
from .encoders import ConformerEncoder, ConformerEncoderInterCTC  # noqa: F401
from .model_ctc import Alignment, HeadMargins, InterCTC, ModelCTC, select_nbest, select_rerun  # noqa: F401
from .transducer import Transducer, TransducerAlignment  # noqa: F401
from .lm import LanguageModel  # noqa: F401
from .checkpoint import load_checkpoint, save_checkpoint  # noqa: F401
from .batching import FrontDoor, bucket_batches, collate_fn_pad  # noqa: F401
from .streaming import RnntStreamState, StreamingCTC, StreamingEncoder, StreamingTransducer, ctc_collapse_carry, stream_align  # noqa: F401

__all__ = ["ConformerEncoder", "ConformerEncoderInterCTC", "ModelCTC", "InterCTC", "model_from_config", "Alignment", "HeadMargins", "select_rerun", "select_nbest", "Transducer", "TransducerAlignment", "LanguageModel", "load_checkpoint", "save_checkpoint", "FrontDoor", "bucket_batches", "collate_fn_pad", "build_plan", "load_config", "named_config", "StreamingEncoder", "StreamingCTC", "StreamingTransducer", "RnntStreamState", "stream_align", "ctc_collapse_carry"]


def model_from_config(cfg, tokenizer=None):
    """The model class the reference's ``model_type`` selects (functions.py:45-66): "CTC" -> ModelCTC, "InterCTC" -> InterCTC, "Transducer" ->
    Transducer, built from a model name, a reference-format JSON path or a dict."""
    cfg = load_config(cfg)
    mtype = cfg.get("model_type", "CTC")
    classes = {"CTC": ModelCTC, "InterCTC": InterCTC, "Transducer": Transducer}
    if mtype not in classes:
        raise Exception("Unknown model type:", mtype)
    return classes[mtype].from_config(cfg, tokenizer)
