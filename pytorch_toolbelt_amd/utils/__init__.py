from .support import *  # noqa: F401,F403
from .torch_utils import *  # noqa: F401,F403
from .rle import *  # noqa: F401,F403
from .metrics import *  # noqa: F401,F403
from .components import *  # noqa: F401,F403
from .distance import *  # noqa: F401,F403
from .surface import *  # noqa: F401,F403
from .instances import *  # noqa: F401,F403
