"""Top-level module name 'trackIdentities' beside the reference's module names (`from trackIdentities import *`): not a module of
the reference -- track identities are an extension -- but scripts that put this directory on PYTHONPATH find
KLTUpdateIdentities and KLTResetIdentities here, and through `from selectGoodFeatures import *` as well.  It *is*
pyfeaturetrack_amd.trackIdentities: the name is aliased, not copied.
"""
import sys

import pyfeaturetrack_amd.trackIdentities as _m

sys.modules[__name__] = _m
