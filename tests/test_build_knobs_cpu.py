"""The library's sources have no build-time experiment switches: the only XDTTS_* names a preprocessor conditional
tests are the three profile builds of `make prof` and the three build-identity macros of build_info.cpp
(DESIGN_NOTES.md, Appendix B)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = {"XDTTS_GL_PROFILE", "XDTTS_PERSIST_PROFILE", "XDTTS_P8_PROFILE"}
IDENTITY = {"XDTTS_SRC_HASH", "XDTTS_BUILD_ARCH", "XDTTS_BUILD_UTC"}


def test_only_the_profile_and_identity_macros_are_tested_by_the_preprocessor():
    found = set()
    for path in glob.glob(os.path.join(ROOT, "xd-tts_amd", "csrc", "*")):
        text = open(path, errors="replace").read().replace("\\\n", " ")
        for line in re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b.*$", text, flags=re.M):
            found |= set(re.findall(r"\bXDTTS_\w+", line))
    assert found == PROFILE | IDENTITY


def test_the_profile_builds_are_built_and_documented():
    make = open(os.path.join(ROOT, "xd-tts_amd", "Makefile")).read()
    rule = re.search(r"^build_prof/%\.o:.*\n((?:\t.*\n)+)", make, flags=re.M).group(1)  # recipe of the prof library's objects
    notes = open(os.path.join(ROOT, "DESIGN_NOTES.md")).read()
    for name in PROFILE:
        assert "-D" + name in rule and name in notes
