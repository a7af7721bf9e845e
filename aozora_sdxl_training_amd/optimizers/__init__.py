from .raven import RavenAdamW
from .titan import TitanAdamW
from .adamw8bit import PagedAdamW8bit
from .prodigy import Prodigy
from .adafactor import Adafactor

__all__ = ["RavenAdamW", "TitanAdamW", "PagedAdamW8bit", "Prodigy", "Adafactor"]
