"""SamplingParams -- the reference's fields and defaults (ssd/sampling_params.py:4-9) plus the truncation every other LLM.generate offers:
top_k / top_p / min_p, applied in the Hugging Face order after the temperature (include/ssd_hip_filter.h has the exact semantics)."""
from dataclasses import dataclass


@dataclass
class SamplingParams:
    temperature: float = 1.0
    draft_temperature: float | None = None
    max_new_tokens: int = 256
    ignore_eos: bool = False
    top_k: int = 0              # keep the k most probable tokens (ties at the k-th kept); 0 = off
    top_p: float = 1.0          # keep the smallest set of most probable tokens whose mass reaches top_p; 1.0 = off
    min_p: float = 0.0          # keep tokens whose probability is at least min_p times the largest; 0.0 = off

    def __post_init__(self):
        if isinstance(self.top_k, bool) or not isinstance(self.top_k, int) or self.top_k < 0:
            raise ValueError(f"top_k must be an integer >= 0 (0 = off), got {self.top_k!r}")
        if not (0.0 < self.top_p <= 1.0):
            raise ValueError(f"top_p must be in (0, 1] (1 = off), got {self.top_p!r}")
        if not (0.0 <= self.min_p <= 1.0):
            raise ValueError(f"min_p must be in [0, 1] (0 = off), got {self.min_p!r}")

    @property
    def active_filters(self) -> list[str]:
        """Names of the truncation parameters that are switched on."""
        return [n for n, on in (("top_k", self.top_k > 0), ("top_p", self.top_p < 1.0), ("min_p", self.min_p > 0.0)) if on]
