"""The HIP sources have two build switches, UDS_PHASE_TIMING and UDS_KNOBS ("Build switches"), and no other
conditional compilation on a UDS_* name: the code the default build compiles is the code in the files."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gnn_uds_amd', 'csrc')
CONDITIONAL = re.compile(r'^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$')


def test_only_the_two_build_switches_are_tested():
    names = {}
    for fn in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, fn)) as f:
            for no, line in enumerate(f, 1):
                m = CONDITIONAL.match(line)
                if m:
                    for name in re.findall(r'\bUDS_\w+', m.group(1).split('//')[0]):
                        names.setdefault(name, []).append('%s:%d' % (fn, no))
    assert set(names) == {'UDS_PHASE_TIMING', 'UDS_KNOBS'}, names
