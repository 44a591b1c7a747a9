# tests/cpp/test_store_plan: the host-only planning of the keypoint pool and the window store
# (form_amd/csrc/store_plan.hpp, no HIP headers), plain g++ -Werror like its neighbours, with
# the address and undefined-behaviour sanitizers (runtimes linked statically: the program needs
# nothing preloaded).
# Built by __graft_entry__.build():  make -C tests/cpp -f store_plan.mk
CXX ?= g++
ROOT := ../..
CXXFLAGS ?= -O1 -g -std=c++17 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all \
	-static-libasan -static-libubsan
all: test_store_plan
test_store_plan: test_store_plan.cpp $(ROOT)/form_amd/csrc/store_plan.hpp
	$(CXX) $(CXXFLAGS) -I$(ROOT)/form_amd/csrc -o $@ test_store_plan.cpp
clean:
	rm -f test_store_plan
.PHONY: all clean
