from .modules import SRLModules  # noqa: F401
from .models import CustomCNN  # noqa: F401
from .supervised import DenseNetwork  # noqa: F401
