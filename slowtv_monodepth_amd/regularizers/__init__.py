from .feature import *  # noqa: F401,F403
from .mask import *  # noqa: F401,F403
from .occlusion import *  # noqa: F401,F403
from .smooth import *  # noqa: F401,F403
