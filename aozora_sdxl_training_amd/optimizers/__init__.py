from .raven import RavenAdamW
from .titan import TitanAdamW
from .adamw8bit import PagedAdamW8bit
from .prodigy import Prodigy

__all__ = ["RavenAdamW", "TitanAdamW", "PagedAdamW8bit", "Prodigy"]
