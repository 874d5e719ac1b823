from pytorch_toolbelt_amd.utils.rle import *  # noqa: F401,F403
from pytorch_toolbelt_amd.utils.rle import __all__  # noqa: F401
