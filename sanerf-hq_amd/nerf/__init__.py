from .network import MLP, NeRFNetwork, SkipConnMLP  # noqa: F401
from .renderer import NeRFRenderer, contract, near_far_from_aabb, sample_pdf  # noqa: F401
from .utils import DeviceCollate, collate_rays, get_rays  # noqa: F401
from .utils import freeze_loaded_parameters, load_checkpoint, save_checkpoint  # noqa: F401
from .sam_cache import SamFeatureCache, feature_map  # noqa: F401
from .mask_step import build_error_map, mask_train_loss  # noqa: F401
from .sam_step import Cache, sam_eval_loss, sam_train_loss, use_cache  # noqa: F401
from .rgb_step import adapt_num_rays, rgb_eval_loss, rgb_train_loss, rgb_train_step, step_background, update_proposal_at  # noqa: F401
from .mask_output import DeviceMeters, mask_eval_step, mask_test_outputs, reference_color_map  # noqa: F401
from .metrics import SSIMMeter  # noqa: F401
from .prompts import PointPrompts, decode_overlay, decode_prompts  # noqa: F401
