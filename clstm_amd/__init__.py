"""clstm_amd -- MI355X-native backing of tmbdev/clstm's LSTM + CTC hot path.

Only what the path needs: csrc/ (hand-written HIP kernels + the C ABI of
include/clstm_abi.h), abi.py (ctypes plumbing), net.py (host mirror of the reference's
INetwork / make_net / sgd_update surface), lm.py (character n-gram models for the beam
search) and lexicon.py (word lists that constrain it).  See DESIGN.md and INTEGRATION.md.
"""
from .abi import ClstmError, load  # noqa: F401
from .lexicon import Lexicon  # noqa: F401
from .lm import CharLM  # noqa: F401
from .net import Degrader, Network, Normalizer, make_net, sgd_update, mktargets, edit_distance, cer  # noqa: F401
